"""ctypes binding of libpf_hip.so (the C ABI declared in include/pf_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent the
import of :mod:`patchfusion_amd.hip_ops` raises.  Build with ``python __graft_entry__.py`` or
``make -C patchfusion_amd/csrc``.
"""
import ctypes as C
import os

# Load order matters: PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 and this library needs the SAME HIP runtime that
# owns torch's streams and device pointers.  With torch imported first the dynamic linker resolves libpf_hip.so's libamdhip64.so.7
# to the copy torch already loaded; dlopen-ing libpf_hip.so first would pull /opt/rocm's runtime into the process next to torch's,
# and every launch on a torch stream then fails (seen as "pf_patch_im2col failed (status 2)" when build() ran before smoke()).
import torch  # noqa: F401  (must precede the CDLL below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PF_LIB_PATH") or os.path.join(_HERE, "libpf_hip.so")   # PF_LIB_PATH: kernel-tuning builds only

vp, ci, cf, cl = C.c_void_p, C.c_int, C.c_float, C.c_long


class ConvParams(C.Structure):
    _fields_ = [
        ("x", vp), ("x_ld", ci), ("B", ci), ("H", ci), ("W", ci), ("Cin", ci),
        ("w", vp), ("w_rows", ci), ("Kpad", ci),
        ("bias", vp), ("scale", vp),
        ("res", vp), ("res_ld", ci), ("res2", vp), ("res2_ld", ci),
        ("y", vp), ("y_ld", ci), ("OH", ci), ("OW", ci), ("Cout", ci),
        ("KH", ci), ("KW", ci), ("stride", ci), ("pad", ci),
        ("act", ci), ("relu_in", ci), ("out_f32", ci), ("shuffle", ci), ("dtype", ci), ("korder", ci),
        ("batch", ci), ("x_bstride", C.c_long), ("w_bstride", C.c_long), ("y_bstride", C.c_long),
        ("col_exp", vp), ("out_exp", vp),
    ]


class JpegHeader(C.Structure):
    """struct pf_jpeg_header of include/pf_hip.h"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "ncomp", "hmax", "vmax", "restart_interval", "orientation", "scan_begin", "mcus_x",
                                         "mcus_y", "blocks_per_mcu", "nblocks", "nsegments", "sof")] + \
               [(n, C.c_int32 * 4) for n in ("comp_id", "comp_h", "comp_v", "comp_tq", "comp_td", "comp_ta")] + \
               [("qt", (C.c_uint8 * 64) * 4), ("qt_present", C.c_uint8 * 4), ("huff_bits", (C.c_uint8 * 17) * 8),
                ("huff_vals", (C.c_uint8 * 256) * 8), ("huff_present", C.c_uint8 * 8)]


class JpegProgScan(C.Structure):
    """struct pf_jpeg_prog_scan of include/pf_hip.h"""
    _fields_ = [("kind", C.c_int32), ("ncomp", C.c_int32), ("comp", C.c_int32 * 4), ("td", C.c_int32 * 4), ("ta", C.c_int32 * 4)] + \
               [(n, C.c_int32) for n in ("ss", "se", "ah", "al", "restart_interval", "begin", "end", "blocks_per_unit", "nblocks", "nsegments",
                                         "blocks_x", "blocks_y")] + \
               [("huff_bits", (C.c_uint8 * 17) * 8), ("huff_vals", (C.c_uint8 * 256) * 8)]


class PngdHeader(C.Structure):
    """struct pf_pngd_header of include/pf_hip.h"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "depth", "color_type", "interlace", "channels", "bpp", "has_trns", "plte_entries",
                                         "idat_chunks")] + \
               [(n, C.c_int64) for n in ("rowbytes", "inflated_bytes", "compressed_bytes")] + [("palette", C.c_uint8 * 768)]


# name -> argtypes (every function returns int status except pf_last_error / pf_version)
SIGNATURES = {
    "pf_conv": [C.POINTER(ConvParams), vp],
    "pf_conv_timed": [C.POINTER(ConvParams), ci, C.POINTER(cf), vp],
    "pf_patch_im2col": [vp, ci, ci, ci, vp, ci, ci, vp],
    "pf_assemble_tokens": [vp, vp, vp, vp, ci, ci, ci, ci, vp],
    "pf_layernorm": [vp, ci, vp, ci, vp, vp, cf, ci, ci, ci, ci, ci, ci, vp],
    "pf_qkv_split": [vp, ci, ci, ci, vp, vp, vp, ci, cf, ci, vp],
    "pf_vit_attention": [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp],
    "pf_vit_attention_qkv": [vp, vp, ci, ci, ci, ci, vp],
    "pf_swin_ln_partition": [vp, ci, vp, vp, vp, cf, ci, ci, ci, ci, ci, ci, vp],
    "pf_swin_window_attention": [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp],
    "pf_swin_unpartition_add": [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp],
    "pf_add_rowwise": [vp, ci, vp, ci, ci, ci, ci, vp],
    "pf_resize_bilinear": [vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, vp, ci, ci, ci, ci, vp],
    "pf_resize_concat": [C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, ci, vp, ci, ci, ci, ci, vp],
    "pf_crop_resize_planar": [vp, ci, ci, ci, vp, ci, vp, ci, ci, vp],
    "pf_roi_align": [vp, ci, ci, ci, ci, ci, vp, ci, vp, ci, ci, ci, cf, ci, ci, ci, vp],
    "pf_maxpool2": [vp, ci, ci, ci, ci, ci, vp, ci, ci, vp],
    "pf_copy_channels": [vp, ci, vp, ci, cl, ci, ci, ci, ci, vp],
    "pf_resize_bilinear_ex": [vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, vp, ci, ci, ci, ci, vp, vp],
    "pf_resize_concat_ex": [C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, ci, vp, ci, ci, ci, ci, vp, vp],
    "pf_roi_align_ex": [vp, ci, ci, ci, ci, ci, vp, ci, vp, ci, ci, ci, cf, ci, ci, ci, vp, vp],
    "pf_copy_channels_ex": [vp, ci, vp, ci, cl, ci, ci, ci, ci, vp, vp],
    "pf_zero_u32": [vp, cl, vp],
    "pf_pack_fusion_input": [vp, vp, vp, vp, ci, ci, ci, ci, vp],
    "pf_nhwc_to_nchw_f32": [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp],
    "pf_conv_winograd": [C.POINTER(ConvParams), ci, vp, ci, ci, vp, vp, vp],
    "pf_conv_winograd_split3": [C.POINTER(ConvParams), vp, ci, ci, vp, vp, vp],
    "pf_conv_winograd_split3_windowed": [C.POINTER(ConvParams), vp, ci, ci, vp, vp, C.c_long, vp],
    "pf_conv_winograd_f16x2_windowed": [C.POINTER(ConvParams), vp, ci, ci, vp, vp, vp, C.c_long, vp],
    "pf_conv_winograd_f16x2_windowed_ex": [C.POINTER(ConvParams), vp, ci, ci, vp, vp, vp, C.c_long, vp, vp, ci, vp],
    "pf_conv_winograd_split3_windowed_ex": [C.POINTER(ConvParams), vp, ci, ci, vp, vp, C.c_long, vp, ci, vp],
    "pf_wino_absmax": [vp, ci, cl, ci, ci, vp, vp],
    "pf_gemm_f16x2_points": [C.POINTER(ConvParams), vp, ci, vp],
    "pf_gemm_f16x2_points128": [C.POINTER(ConvParams), vp, ci, vp],
    "pf_gemm_f16x2_points160": [C.POINTER(ConvParams), vp, ci, vp],
    "pf_gemm_f16x2": [C.POINTER(ConvParams), vp],
    "pf_gemm_split3": [C.POINTER(ConvParams), vp],
    "pf_gemm_split3_ex": [C.POINTER(ConvParams), ci, vp],
    "pf_conv1x1_split3": [C.POINTER(ConvParams), vp, ci, vp],
    "pf_gemm_split3_timed": [C.POINTER(ConvParams), ci, C.POINTER(cf), vp],
    "pf_gemm_bf16_pp": [C.POINTER(ConvParams), vp],
    "pf_split3": [vp, ci, vp, ci, cl, cl, ci, vp],
    "pf_layernorm_split3": [vp, ci, vp, ci, cl, ci, vp, vp, cf, cl, ci, vp],
    "pf_layernorm_f16x2": [vp, ci, vp, vp, vp, vp, cf, cl, ci, vp],
    "pf_vit_attention_qkv_split3": [vp, vp, cl, ci, ci, ci, ci, vp],
    "pf_vit_attention_split3": [vp, cl, vp, cl, ci, ci, ci, ci, vp],
    "pf_vit_attention_split3_v2": [vp, cl, vp, cl, ci, ci, ci, ci, ci, ci, vp],
    "pf_vit_attention_f16x2": [vp, cl, vp, vp, cl, vp, ci, ci, ci, vp],
    "pf_vit_attention_split3_rpb": [vp, cl, vp, cl, ci, ci, ci, ci, vp, ci, ci, ci, vp],
    "pf_patch_im2col_norm": [vp, ci, ci, ci, ci, vp, vp, vp, ci, vp],
    "pf_readout_concat": [vp, ci, ci, ci, ci, vp, ci, vp],
    "pf_vit_attention_rpb_bf16": [vp, vp, vp, vp, ci, ci, ci, ci, vp, ci, ci, vp],
    "pf_patch_im2col_norm_bf16": [vp, ci, ci, ci, ci, vp, vp, vp, ci, vp],
    "pf_readout_concat_bf16": [vp, ci, ci, ci, ci, vp, ci, vp],
    "pf_conv_winograd_fused": [C.POINTER(ConvParams), vp, ci, ci, vp],
    "pf_conv_winograd_fused_timed": [C.POINTER(ConvParams), vp, ci, ci, ci, C.POINTER(cf), vp],
    "pf_attractor": [vp, ci, ci, ci, cf, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, vp],
    "pf_seed_bin_centers": [vp, ci, vp, cl, ci, cf, cf, ci, ci, vp],
    "pf_bounded_bin_centers": [vp, vp, cl, ci, cf, cf, vp],
    "pf_logbinom_depth": [vp, ci, vp, ci, ci, vp, ci, ci, ci, ci, cf, cf, vp],
    "pf_bins_tail": [vp, ci, ci, vp, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, cf, cf, vp],
    "pf_stitch_init": [vp, vp, ci, ci, vp, vp, vp, ci, ci, ci, vp],
    "pf_stitch_finish_init": [vp, vp, vp, cl, vp],
    "pf_stitch_update": [vp, vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, vp],
    "pf_resize_nearest_f32": [vp, ci, ci, vp, ci, ci, vp],
    "pf_resize_bilinear_f32": [vp, ci, ci, vp, ci, ci, vp],
    # input / output side (io.hip)
    "pf_u8_bicubic_to_f32": [vp, ci, ci, ci, vp, ci, ci, vp],
    "pf_percentiles_f32": [vp, cl, cf, ci, vp, C.c_double, C.c_double, vp, vp, vp],
    "pf_colorize_f32": [vp, cl, vp, vp, ci, cf, ci, vp, C.c_uint32, vp, vp],
    "pf_depth_to_u16": [vp, cl, cf, vp, vp],
    "pf_silog_loss": [vp, vp, cl, cf, cf, cf, vp, vp, vp],
    "pf_depth_metrics": [vp, ci, ci, vp, ci, ci, vp, vp, cf, cf, ci, ci, ci, ci, vp, vp],
    "pf_depth_boundaries": [vp, ci, ci, ci, cf, ci, vp, vp],
    "pf_colorize_f32_ex": [vp, cl, vp, vp, ci, cf, ci, vp, C.c_uint32, ci, vp, vp],
    # PNG encoding of the saved images (png.hip); pf_png_build_table is host-only: host pointers, no GPU call
    "pf_png_workspace_bytes": [ci, ci, ci, ci, C.POINTER(cl), C.POINTER(cl), C.POINTER(ci)],
    "pf_png_filter_histogram": [vp, ci, ci, ci, ci, ci, vp, vp, vp],
    "pf_png_build_table": [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "pf_png_encode": [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp],
    # the same with run matches (png_rle.hip); pf_png_rle_build_table is host-only too
    "pf_png_rle_workspace_bytes": [ci, ci, ci, ci, C.POINTER(cl), C.POINTER(cl), C.POINTER(ci)],
    "pf_png_rle_filter_histogram": [vp, ci, ci, ci, ci, ci, vp, vp, vp],
    "pf_png_rle_build_table": [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "pf_png_rle_encode": [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp],
    # JPEG decoding of the input image (jpeg.hip); parse, prepare_scan, decode_entropy_host, plan and build_tables are host-only
    "pf_jpeg_parse": [vp, cl, C.POINTER(JpegHeader)],
    "pf_jpeg_prepare_scan": [vp, cl, C.POINTER(JpegHeader), vp, cl, C.POINTER(cl), vp],
    "pf_jpeg_decode_entropy_host": [C.POINTER(JpegHeader), vp, cl, vp, vp],
    "pf_jpeg_plan": [C.POINTER(JpegHeader), vp, ci, vp, cl, vp, C.POINTER(ci), C.POINTER(ci)],
    "pf_jpeg_build_tables": [C.POINTER(JpegHeader), vp],
    "pf_jpeg_workspace_bytes": [C.POINTER(JpegHeader), ci, C.POINTER(cl), C.POINTER(cl)],
    "pf_jpeg_decode_entropy": [C.POINTER(JpegHeader), vp, cl, vp, vp, ci, ci, vp, ci, vp, vp, C.POINTER(ci), vp],
    "pf_jpeg_reconstruct": [C.POINTER(JpegHeader), vp, ci, vp, vp, vp],
    # progressive JPEG (jpeg_prog.hip); decode_scan, dc_refine, nonzero_mask and apply_refinement launch kernels, the rest is host-only
    "pf_jpeg_prog_parse": [vp, cl, C.POINTER(JpegHeader), C.POINTER(JpegProgScan), ci, C.POINTER(ci)],
    "pf_jpeg_prog_prepare_scan": [vp, cl, C.POINTER(JpegProgScan), vp, cl, C.POINTER(cl), vp],
    "pf_jpeg_prog_decode_scan_host": [C.POINTER(JpegHeader), C.POINTER(JpegProgScan), vp, cl, vp, vp],
    "pf_jpeg_prog_refine_ac_host": [C.POINTER(JpegProgScan), vp, cl, vp, vp, vp],
    "pf_jpeg_prog_plan": [C.POINTER(JpegProgScan), vp, ci, vp, cl, vp, C.POINTER(ci), C.POINTER(ci)],
    "pf_jpeg_prog_build_tables": [C.POINTER(JpegProgScan), vp],
    "pf_jpeg_prog_block_map": [C.POINTER(JpegHeader), C.POINTER(JpegProgScan), vp],
    "pf_jpeg_prog_workspace_bytes": [ci, ci, C.POINTER(cl)],
    "pf_jpeg_prog_decode_scan": [C.POINTER(JpegHeader), C.POINTER(JpegProgScan), vp, cl, vp, vp, ci, ci, vp, vp, ci, vp, vp, C.POINTER(ci), vp],
    "pf_jpeg_prog_dc_refine": [C.POINTER(JpegHeader), C.POINTER(JpegProgScan), vp, cl, vp, vp, vp, vp],
    "pf_jpeg_prog_nonzero_mask": [C.POINTER(JpegHeader), C.POINTER(JpegProgScan), vp, vp, vp, vp],
    "pf_jpeg_prog_apply_refinement": [C.POINTER(JpegHeader), C.POINTER(JpegProgScan), vp, vp, vp, vp],
    # PNG decoding of the input image (png_decode.hip); parse and the *_host entry points are host-only
    "pf_pngd_parse": [vp, cl, ci, C.POINTER(PngdHeader), vp, cl, C.POINTER(cl)],
    "pf_pngd_find_host": [vp, cl, C.c_uint32, vp, cl, C.POINTER(cl)],
    "pf_pngd_scan_host": [vp, cl, C.c_uint32, vp, ci, C.c_uint32, C.c_uint32, vp],
    "pf_pngd_inflate_model_host": [vp, cl, cl, C.c_uint32, vp, vp],
    "pf_pngd_find": [vp, cl, C.c_uint32, vp, C.c_uint32, vp, vp],
    "pf_pngd_scan": [vp, cl, C.c_uint32, vp, ci, C.c_uint32, C.c_uint32, vp, vp],
    "pf_pngd_inflate": [vp, cl, C.c_uint32, vp, ci, C.c_uint32, vp, vp, vp, vp],
    "pf_pngd_resolve": [vp, vp, C.c_uint32, ci, vp, vp],
    "pf_pngd_unfilter": [vp, C.POINTER(PngdHeader), vp, vp, vp],
    "pf_pngd_expand": [vp, C.POINTER(PngdHeader), vp, vp, vp, vp],
    "pf_pngd_adler": [vp, cl, vp, vp, vp],
    "pf_pngd_to_rgb8": [vp, ci, ci, ci, ci, vp, vp],
    "pf_pngd_scan_par_host": [vp, cl, C.c_uint32, vp, ci, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp],
    "pf_pngd_inflate_par_host": [vp, cl, C.c_uint32, vp, ci, C.c_uint32, C.c_uint32, vp, vp, vp, vp],
    "pf_pngd_scan_par": [vp, cl, C.c_uint32, vp, ci, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp],
    "pf_pngd_inflate_par": [vp, cl, C.c_uint32, vp, ci, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp],
    # ground-truth depth files (gtread.hip)
    "pf_gt_convert": [vp, ci, ci, ci, ci, ci, cf, cf, vp, vp, vp],
    # training-side augmentations (augment.hip); m, colour and a are host arrays
    "pf_aug_image_u8_to_f32": [vp, ci, ci, C.POINTER(C.c_double), ci, ci, cf, cf, C.POINTER(C.c_double), vp, vp],
    "pf_aug_planes_nearest": [vp, vp, ci, ci, C.POINTER(ci), ci, vp, vp, vp],
    # backward of the metric-bins head and of the SILog loss (head_bwd.hip)
    "pf_conv1x1_wgrad_workspace_bytes": [cl, ci, ci, ci, C.POINTER(cl)],
    "pf_conv1x1_wgrad": [vp, ci, vp, ci, cl, ci, ci, vp, vp, vp, cl, ci, vp],
    "pf_resize_bilinear_bwd": [vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, vp],
    "pf_attractor_bwd": [vp, ci, ci, ci, ci, vp, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, vp],
    "pf_logbinom_depth_bwd": [vp, ci, vp, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, cf, cf, vp, vp],
    "pf_act_bwd": [vp, ci, vp, ci, cl, ci, ci, vp],
    "pf_silog_loss_bwd": [vp, vp, cl, cf, cf, cf, vp, cf, vp, vp],
}
NON_STATUS = ("pf_last_error", "pf_version", "pf_percentile_workspace_bytes", "pf_conv_winograd_fused_supported", "pf_gemm_split3_route",
              "pf_gemm_f16x2_points_route", "pf_gemm_f16x2_points_route_ex", "pf_gemm_f16x2_route", "pf_wino_f16x2_tile_route", "pf_conv_winograd_f16x2_supported_ex",
              "pf_wino_f16x2_scratch_bytes", "pf_conv_winograd_f16x2_supported", "pf_vit_attention_rpb_bf16_lds_bytes",
              "pf_conv_last_variant", "pf_pngd_par_window", "pf_persist_grid")   # entry points that do not return a status

_lib = None


def load():
    """Load the shared library and bind every symbol of the C ABI; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python __graft_entry__.py` "
            "(or `make -C patchfusion_amd/csrc`). There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.argtypes = args
        fn.restype = ci
    lib.pf_last_error.restype = C.c_char_p
    lib.pf_last_error.argtypes = []
    lib.pf_version.restype = ci
    lib.pf_version.argtypes = []
    lib.pf_percentile_workspace_bytes.restype = ci
    lib.pf_percentile_workspace_bytes.argtypes = []
    lib.pf_conv_winograd_fused_supported.restype = ci          # 1 / 0, not a status
    lib.pf_conv_winograd_fused_supported.argtypes = [C.POINTER(ConvParams)]
    lib.pf_gemm_split3_route.restype = ci                      # PF_S3_ROUTE_* (or -1), not a status
    lib.pf_gemm_split3_route.argtypes = [C.POINTER(ConvParams), ci]
    lib.pf_gemm_f16x2_points_route.restype = ci                # PF_S3_ROUTE_PERSIST192 / PERSIST128 (or -1), not a status
    lib.pf_gemm_f16x2_points_route.argtypes = [C.POINTER(ConvParams), ci]
    lib.pf_gemm_f16x2_points_route_ex.restype = ci             # the same, for a layer whose channel maxima are handed in
    lib.pf_gemm_f16x2_points_route_ex.argtypes = [C.POINTER(ConvParams), ci, ci]
    lib.pf_gemm_f16x2_route.restype = ci                       # PF_S3_ROUTE_PERSIST192 / TILE160 (or -1): the tile form of an fp16x2 linear
    lib.pf_gemm_f16x2_route.argtypes = [C.POINTER(ConvParams), ci]
    lib.pf_wino_f16x2_tile_route.restype = ci                  # 1 = the 160 x 256 tile, 0 = the form the points route names (or -1), not a status
    lib.pf_wino_f16x2_tile_route.argtypes = [C.POINTER(ConvParams), ci]
    lib.pf_persist_grid.restype = ci                           # blocks of a persistent GEMM (0 = one-tile kernel, -1 = refused), not a status
    lib.pf_persist_grid.argtypes = [ci, ci, C.c_long, ci]
    lib.pf_conv_winograd_f16x2_supported_ex.restype = ci              # 1 / 0, not a status
    lib.pf_conv_winograd_f16x2_supported_ex.argtypes = [C.POINTER(ConvParams), ci, ci, C.c_long, ci]
    lib.pf_wino_f16x2_scratch_bytes.restype = C.c_long                 # bytes, not a status
    lib.pf_wino_f16x2_scratch_bytes.argtypes = [ci, ci]
    lib.pf_conv_winograd_f16x2_supported.restype = ci                 # 1 / 0, not a status
    lib.pf_conv_winograd_f16x2_supported.argtypes = [C.POINTER(ConvParams), ci, ci, C.c_long]
    lib.pf_vit_attention_rpb_bf16_lds_bytes.restype = ci              # bytes (or -1), not a status
    lib.pf_vit_attention_rpb_bf16_lds_bytes.argtypes = [ci, ci, ci]
    lib.pf_conv_last_variant.restype = ci                             # variant code of the thread's last pf_conv launch, not a status
    lib.pf_conv_last_variant.argtypes = []
    lib.pf_pngd_par_window.restype = ci                               # lanes per window of the subsequence inflate, not a status
    lib.pf_pngd_par_window.argtypes = []
    _lib = lib
    return lib


class PfError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        msg = load().pf_last_error()
        raise PfError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")
