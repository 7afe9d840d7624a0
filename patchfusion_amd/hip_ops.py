"""Typed Python wrappers over the C ABI (include/pf_hip.h).

Every function takes torch tensors that live on the GPU, extracts raw device pointers / strides and
launches the hand-written HIP kernel on torch's *current* stream.  PyTorch is used for memory and
streams only.  There is no CPU path here: CPU tensors are rejected and a missing shared library
makes this module fail to import (see _lib.load).

Tensor conventions: activations are NHWC views ``[B,H,W,C]`` (or token matrices ``[M,C]``) with
unit channel stride; the pixel stride (``ld``) may exceed C when the tensor is a channel slice of a
concat buffer.  dtype float32 = exact mode, bfloat16 = fast mode; a few head tensors are always f32.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ConvParams, check
from .packing import PackedConv, winograd_applies

_L = _lib.load()

ACT = {"none": 0, None: 0, "relu": 1, "gelu": 2, "softplus": 3}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.PfError("patchfusion_amd.hip_ops: tensor is not on the GPU (there is no CPU path)")
    if t.device.index != torch.cuda.current_device():
        # kernels are launched on torch's CURRENT device/stream; a tensor of another GPU would be accessed through the
        # wrong context (and the >64 KiB LDS opt-in is per device): make the mismatch loud instead
        raise _lib.PfError(f"patchfusion_amd.hip_ops: tensor lives on cuda:{t.device.index} but the current device is "
                           f"cuda:{torch.cuda.current_device()} (wrap the call in torch.cuda.device(...))")
    return C.c_void_p(t.data_ptr())


def _dt(t):
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise _lib.PfError(f"unsupported dtype {t.dtype}")


def _as4(t):
    if t.dim() == 2:
        return t.unsqueeze(0).unsqueeze(0)
    if t.dim() == 3:
        return t.unsqueeze(0)
    return t


def _ld(t):
    """pixel stride of a dense-in-(B,H,W) NHWC view"""
    t = _as4(t)
    B, H, W, Cc = t.shape
    assert t.stride(3) == 1, "channel stride must be 1"
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else max(Cc, t.stride(2)))
    if W > 1 and H > 1:
        assert t.stride(1) == W * ld, "rows must be dense"
    if B > 1:
        assert t.stride(0) == H * W * ld, "batches must be dense"
    return ld


_LOGC = {}


def _logbinom_logc(n_bins, device):
    """log C(n_bins - 1, k), k = 0 .. n_bins - 1, as the reference computes it (dist_layers.py:29-45: float32 tensor arithmetic in torch, Stirling
    form with eps = 1e-7), once per (n_bins, device): constants of the model, handed to pf_logbinom_depth_bwd (include/pf_hip.h says why)"""
    key = (int(n_bins), device)
    if key not in _LOGC:
        eps = 1e-7
        k = torch.arange(n_bins, dtype=torch.float32) + eps
        n = torch.full((1,), float(n_bins - 1)) + eps
        _LOGC[key] = (n * torch.log(n) - k * torch.log(k) - (n - k) * torch.log(n - k + eps)).to(device)
    return _LOGC[key]


_ENV = {}


def _env(name, default):
    """PF_* switch, resolved ONCE (first use after import / refresh_env) instead of on every library call: round 3 read 4-6 environment
    variables per convolution, ~20 % of the 22 us the Python host spent per call (tools/host_overhead.py)."""
    v = _ENV.get(name)
    if v is None:
        import os
        v = _ENV[name] = os.environ.get(name, default)
    return v


def refresh_env():
    """forget every cached PF_* switch and every cached dispatch decision (called by the engine build and by tests that flip switches)"""
    _ENV.clear()
    _CONV_CACHE.clear()


_CONV_CACHE = {}


def _bf16_pp_enabled():
    """plain bf16 linears through the split GEMM's ping-pong pipeline (pf_gemm_bf16_pp, 256 x 128 tiles): measured and NOT kept -- 0.095 /
    0.047 / 0.118 / 0.126 ms on the ViT-L qkv / proj / fc1 / fc2 shapes against 0.086 / 0.038 / 0.108 / 0.105 for the implicit-GEMM kernels
    (profiles/r3_bf16_pp_sweep.log): one product per fragment pair does not amortise the pipeline the way the split GEMM's six do.
    PF_BF16_PP=1 turns it on (A/B, tests/op_checks.py conv_bf16_pp)."""
    return _env("PF_BF16_PP", "0") == "1"


def _conv1x1_split3_wanted(M, pw):
    """float32 1x1 layer through csrc/conv1x1_split3.hip (persistent walk of 64 x 128 tiles, two blocks per CU) instead of the f32-MFMA implicit GEMM?
    PF_CONV1X1_SPLIT3: 0 = never, 2 = wherever the planes exist, 1 (default) = the measured rule (profiles/r6_conv1x1_split3.md: 1.23-1.55x on every layer
    of the pass with at least 64 output channels and two tiles per CU, incl. the 32 -> 96 / 128 linears of the first G2L level; 0.78x on 128 -> 32 and
    1.06x on 32 -> 32, where a 128-wide channel tile multiplies zeros)."""
    mode = _env("PF_CONV1X1_SPLIT3", "1")
    if mode == "0":
        return False
    if mode == "2":
        return True
    tiles = -(-M // 64) * -(-pw.cout // 128)
    return tiles >= 512 and pw.cout >= 64


def conv1x1_split3_layout_ok(pw, x_ptr, x_ld, y_ptr, y_ld, res_ptr=None, res_ld=0, res2_ptr=None, res2_ld=0):
    """the layout rule of csrc/conv1x1_split3.hip (pf_conv1x1_split3), on pointer values and pixel strides in floats: float4 loads and stores need
    x, y, res, res2 (and the packed bias / scale) on 16-byte boundaries and every ld a multiple of 4; x_ld >= Cin, Cin % 32 == 0, Cout % 4 == 0"""
    if pw.w3 is None or pw.cin % 32 or pw.cout % 4 or x_ld < pw.cin or y_ld < pw.cout:
        return False
    ptrs = [x_ptr, y_ptr, pw.w3.data_ptr()] + [t.data_ptr() for t in (pw.bias, pw.scale) if t is not None]
    lds = [x_ld, y_ld]
    for ptr, ld in ((res_ptr, res_ld), (res2_ptr, res2_ld)):
        if ptr is not None:
            ptrs.append(ptr)
            lds.append(ld)
    return all(v % 16 == 0 for v in ptrs) and all(v % 4 == 0 for v in lds)


def _split3_three_step(pw):
    """does the three-step form of this layer run its GEMM in split precision? (filters packed as three planes and PF_WINO_SPLIT3 != 0)"""
    return pw.wino_u3 is not None and _env("PF_WINO_SPLIT3", "1") != "0"


def _wino_f16x2_enabled():
    """three-step split layers whose product runs on the 192 x 192 kernel take its fp16x2 form (csrc/wino_f16x2.hip: two fp16 planes per operand with
    power-of-two channel / column scales, three MFMAs per product instead of six), and so do the 128-tile layers the rule of
    pf_gemm_f16x2_points_route picks (csrc/wino_f16x2_n256.hip; PF_WINO_F16X2_N256=0 / 2, read by the library); PF_WINO_F16X2=0 keeps every layer
    on the bf16x3 planes"""
    return _env("PF_WINO_F16X2", "1") != "0"


def _fused_wanted(B, H, W, pw):
    """Fused Winograd kernel (csrc/wino_fused.hip) or the three-step form for this call?  PF_WINO_FUSED (read per call): 0 = never fused,
    2 = fused wherever supported, 1 (default) = the measured rule (profiles/r3_wino_fused_layers.log, r3_three_step_split.log; 1x MI355X):
    the fused kernel needs at least two rounds of blocks, and it loses to the three-step form on layers with MANY OUTPUT CHANNELS -- each of
    the ceil(Cout/64) channel blocks repeats the input transform, while the batched GEMM of the three-step form runs near its peak there:
    with the split-precision GEMM from 256 output channels on (round 3: 512; 544->544 @ 8x392x518: 16.3 vs 22.5 ms; 768->768 @ 8x224x296: 8.4 vs 13.5),
    with the f32 GEMM only at 768+ -> 768+ (13.0 vs 13.5).  Below that the fused kernel wins 1.1x (768->256) ... 2.4x (-> 32 channels)."""
    mode = _env("PF_WINO_FUSED", "1")
    if mode == "0":
        return False
    if mode == "2":
        return True
    th, tw = -(-H // 4), -(-W // 4)
    nsuper = B * min(-(-th // 4) * -(-tw // 8), -(-th // 8) * -(-tw // 4))
    if pw.wino_u is None:
        many_out = False                                    # fused-only layer: the alternative is the direct kernel
    elif _split3_three_step(pw):
        # round 4 (persistent split GEMM on chunk-major planes, profiles/r4_fused_vs_three_step.md): three steps win 1.04 .. 1.9x from 256 output
        # channels on (768->256 @ 8x224x296: 3.87 vs 4.84 ms), the fused kernel keeps 256->128 (0.91x) and the 32-channel layers (0.4x)
        many_out = pw.cout >= 256
    else:
        many_out = pw.cin >= 768 and pw.cout >= 768
    return nsuper * -(-pw.cout // 64) >= 512 and not many_out


_WS = {}
_WS16 = {}


def _workspace(device, nV, nM):
    """V / M workspaces of the three-step Winograd path, one growing pair per (device, stream): launches of one stream are ordered, so
    the pair can be reused by every layer of that stream instead of 2 x 8 GB of fresh allocations per call (round-2 advisor finding).
    Growth drops the old buffer BEFORE allocating the larger one (round-3 advisor finding: `v = None` only cleared the local name, the dict
    still held the old buffer, so old and new coexisted); release_workspaces() frees everything (model teardown / `_apply`)."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    v, m = _WS.get(key, (None, None))
    if v is None or v.numel() < nV or m is None or m.numel() < nM:
        _WS.pop(key, None)
        if v is None or v.numel() < nV:
            v = None
            v = torch.empty(nV, dtype=torch.float32, device=device)
        if m is None or m.numel() < nM:
            m = None
            m = torch.empty(nM, dtype=torch.float32, device=device)
        _WS[key] = (v, m)
    return v, m


def _f16x2_scratch(device, nbytes):
    """per-(device, stream) scratch of the fp16x2 Winograd layers: channel maxima, scaled filter planes, column exponents (rewritten by every call)"""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    t = _WS16.get(key)
    if t is None or t.numel() < nbytes:
        _WS16.pop(key, None)
        t = None
        t = _WS16[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


_WSCMAX = {}


def _cmax_buffer(device, n, slot="t"):
    """per-(device, stream, slot) uint32 buffer for the channel maxima handed to an fp16x2 layer by the kernels that write its input: slot "t" = the
    intermediate of a conv_chain (filled by conv 1's output transform); the other slots are named by the caller of cmax_begin, one per input tensor
    that is alive at the same time (launches of one stream are ordered, so a slot is free again once its consumer has been launched)"""
    key = (device.index, torch.cuda.current_stream().cuda_stream, slot)
    t = _WSCMAX.get(key)
    if t is None or t.numel() < n:
        t = _WSCMAX[key] = torch.empty(max(n, 1024), dtype=torch.int32, device=device)
    return t


def _cmax_handover_enabled():
    """PF_WINO_F16X2_N256=2 (and 0): every fp16x2 layer runs its own range pass (A/B of the hand-over alone); 5: the hand-over, and the 128-tile
    layers whose maxima are given take fp16x2 from K >= 256 and 2128 tiles on (measured, not adopted: csrc/gemm_split3.hip f16x2_points_route)"""
    return _env("PF_WINO_F16X2_N256", "1") not in ("0", "2")


def _cmax_ptr(cmax, n):
    """device pointer of a uint32 channel-maxima vector (int32 storage, unit stride, at least n entries), or None"""
    if cmax is None:
        return None
    assert cmax.dtype == torch.int32 and cmax.dim() == 1 and cmax.stride(0) == 1 and cmax.numel() >= n, (cmax.dtype, cmax.shape, n)
    return _p(cmax)


def release_workspaces():
    """free the per-(device, stream) Winograd arenas (at the headline layer 12 GB + 8 GB per stream); they are re-grown on demand.  Also drops the
    cached dispatch plans: they hold strong references to the packed layers (device weights + Winograd filter planes, several GB for ViT-L), so
    `del model; release_workspaces(); torch.cuda.empty_cache()` really returns the memory (round-4 advisor finding)"""
    _WS.clear()
    _WS16.clear()
    _WSCMAX.clear()
    _CONV_CACHE.clear()


def workspace_bytes():
    return sum(v.numel() * 4 + m.numel() * 4 for v, m in _WS.values()) + sum(t.numel() for t in _WS16.values())


def _fused_group():
    """PF_WINO_GS: super-tiles per block group (L2 locality knob); PF_WINO_SHAPE: 0 = automatic, 8 | 4 = forced super-tile width (tuning)"""
    return ((int(_env("PF_WINO_GS", "8")) & 0xffff) | (int(_env("PF_WINO_SHAPE", "0")) << 16)
            | (int(_env("PF_WINO_DBG", "0")) << 20))     # PF_WINO_DBG: timing decomposition only (wrong results), see wino_fused.hip


def wino3_window(B, H, W, pw):
    """(window, nwin, nV, nM): a three-step split-precision Winograd layer over T = B ceil(H/4) ceil(W/4) tiles runs `window` tiles at a time (nwin
    windows, the last one ragged) through ONE arena pair of nV + nM float32 words (V: three bf16 planes; M: float32) -- csrc/winograd.hip run_split3.
    Winograd tiles are independent, so the numbers are identical for every window.  PF_WS_CAP_GB (default 2.5) is the largest V + M pair a layer may ask
    for; windows are multiples of 192 tiles (the GEMM's token tile).  The headline layer (544->544 @ 8 x 392 x 518: 11.9 + 8.0 GB per stream in one piece)
    runs in 8 windows of 2.3 GB.  Measured (profiles/r5_ws_cap.md, r5_subbatch_probe.md): the batched GEMM keeps its rate (0.555 of 2500/6 at 8 tiles of
    392 x 518 per launch, 0.551 at 2, 0.538 at 1), and the IMAGE pass gets faster -- 188.6 ms in one piece, 187.3 at 5 GB, 186.4 at 2.5 GB: the two tile
    streams interleave at a finer grain -- while the peak allocation falls from 62.8 to 31 GiB."""
    T = B * -(-H // 4) * -(-W // 4)
    per_tile = 36 * (pw.cin * 6 + pw.cout * 4)
    cap = float(_env("PF_WS_CAP_GB", "2.5")) * 2 ** 30
    window = max(int(cap // per_tile) // 192 * 192, 192)
    if window >= T:
        window = -(-T // 8) * 8
    nwin = -(-T // window)
    return window, nwin, (36 * window * pw.cin * 3 + 1) // 2, 36 * window * pw.cout


def last_conv_variant():
    """code of the kernel variant the calling thread's last pf_conv launched (include/pf_hip.h pf_conv_last_variant: family, tile shape, shuffle,
    RELU_IN); 0 before the first launch.  For the tests (tests/test_bf16_grade_gpu.py): nothing on the product path reads it."""
    return int(_L.pf_conv_last_variant())


def _align16(*ts):
    """the 16-byte alignment of each tensor's data pointer: part of the plan key, because the route may depend on it (conv1x1_split3_layout_ok)"""
    return tuple(None if t is None else t.data_ptr() % 16 for t in ts)


class HipOps:
    name = "hip"

    # ---------------- allocation ----------------
    @staticmethod
    def empty(shape, dtype, device):
        return torch.empty(shape, dtype=dtype, device=device)

    @staticmethod
    def zeros(shape, dtype, device):
        return torch.zeros(shape, dtype=dtype, device=device)

    # ---------------- conv / linear ----------------
    @staticmethod
    def _conv_plan(x, pw, y, stride, pad, act, relu_in, res, res2, direct, given=False):
        """everything about a conv call that does not change while shapes / strides / the packed layer stay the same: the argument checks, the filled
        pf_conv_params and the dispatch decision ('pp' | 's3_1x1' | 'fused' | 'wino3h' | 'wino3' | 'wino' | 'direct').  Cached by HipOps.conv per (layer, layout).
        given: the call will hand in the channel maxima of x (cmax_in) -- the route then follows pf_gemm_f16x2_points_route_ex (the same layers at
        default switches; more 128-tile layers under PF_WINO_F16X2_N256=5)."""
        x4, y4 = _as4(x), _as4(y)
        B, H, W, _ = x4.shape
        OH = (H + 2 * pad - pw.KH) // stride + 1
        OW = (W + 2 * pad - pw.KW) // stride + 1
        s = pw.shuffle
        assert y4.shape[0] == B and y4.shape[1] == OH * s and y4.shape[2] == OW * s, (x4.shape, y4.shape, OH, OW, s)
        assert x4.shape[3] >= pw.cin and y4.shape[3] >= pw.cout // (s * s), (x4.shape, y4.shape, pw.cin, pw.cout)
        p = ConvParams()
        p.x, p.x_ld, p.B, p.H, p.W, p.Cin = x4.data_ptr(), _ld(x4), B, H, W, pw.cin
        p.w, p.w_rows, p.Kpad = pw.w.data_ptr(), pw.w.shape[0], pw.w.shape[1]
        p.bias = pw.bias.data_ptr() if pw.bias is not None else None
        p.scale = pw.scale.data_ptr() if pw.scale is not None else None
        p.res = res.data_ptr() if res is not None else None
        p.res_ld = _ld(res) if res is not None else 0
        p.res2 = res2.data_ptr() if res2 is not None else None
        p.res2_ld = _ld(res2) if res2 is not None else 0
        p.y, p.y_ld, p.OH, p.OW, p.Cout = y4.data_ptr(), _ld(y4), OH, OW, pw.cout
        p.KH, p.KW, p.stride, p.pad = pw.KH, pw.KW, stride, pad
        p.act, p.relu_in = ACT[act], int(bool(relu_in))
        p.dtype = _dt(x4)
        assert pw.w.dtype == x4.dtype, "weights must be packed in the activation dtype"
        p.out_f32 = int(y4.dtype == torch.float32 and x4.dtype != torch.float32)
        p.shuffle = s
        p.korder = pw.korder
        for t in (x4, y4, pw.w, res, res2):
            _p(t)
        f32_io = y4.dtype == torch.float32 and (res is None or res.dtype == torch.float32) and (res2 is None or res2.dtype == torch.float32)
        if (x4.dtype == torch.bfloat16 and pw.KH == 1 and pw.KW == 1 and stride == 1 and pad == 0 and s == 1 and not relu_in and not direct and
                B * H * W >= 2048 and pw.cin % 64 == 0 and pw.cin >= 512 and pw.cout >= 512 and _bf16_pp_enabled()):
            # bf16 linear layers with many token rows (ViT blocks, DPT projections): 256 x 128 ping-pong tiles (csrc/gemm_split3.hip, PLAIN)
            return "pp", p, None
        if (pw.w3 is not None and x4.dtype == torch.float32 and f32_io and stride == 1 and pad == 0 and s == 1 and not direct and
                conv1x1_split3_layout_ok(pw, p.x, p.x_ld, p.y, p.y_ld, p.res, p.res_ld, p.res2, p.res2_ld) and _conv1x1_split3_wanted(B * H * W, pw)):
            # float32 1x1 layers with enough tokens: split-precision product on the bf16 matrix cores, x split in the kernel's loader
            return "s3_1x1", p, (_p(pw.w3), pw.w3.shape[2])
        wino = winograd_applies(pw, B * H * W, stride, pad, act) and not direct
        if wino and pw.wino_up is not None and _fused_wanted(B, H, W, pw) and _L.pf_conv_winograd_fused_supported(C.byref(p)):
            # fused F(4x4,3x3): one kernel, no V / M workspaces (csrc/wino_fused.hip)
            assert f32_io
            return "fused", p, (_p(pw.wino_up), pw.wino_up.shape[0], _fused_group())
        if wino and pw.wino_u is not None:
            # float32 3x3 layers: input transform -> (m+2)^2 GEMMs -> output transform (csrc/winograd.hip)
            m = pw.wino_m
            T = B * -(-H // m) * -(-W // m)
            a2 = (m + 2) ** 2
            assert f32_io
            if m == 4 and _split3_three_step(pw):
                # (split: V holds three bf16 planes = 6 bytes per element instead of 4; whole tile octets, csrc/winograd.hip)
                window, _, nV, nM = wino3_window(B, H, W, pw)
                rows, kpad = pw.wino_u.shape[1], pw.wino_u.shape[2]
                if _wino_f16x2_enabled() and _L.pf_conv_winograd_f16x2_supported_ex(C.byref(p), rows, kpad, window, int(bool(given))):
                    # fp16x2 planes (the same windows; V: two fp16 planes = one float32 word per element)
                    return "wino3h", p, (_p(pw.wino_u), rows, kpad, 36 * window * pw.cin, nM, window, _L.pf_wino_f16x2_scratch_bytes(pw.cin, rows))
                return "wino3", p, (_p(pw.wino_u3), pw.wino_u3.shape[3], pw.wino_u3.shape[2] * 32, nV, nM, window)
            return "wino", p, (m, _p(pw.wino_u), pw.wino_u.shape[1], pw.wino_u.shape[2], a2 * T * pw.cin, a2 * T * pw.cout)
        return "direct", p, None          # (incl. fused-only layers below the block threshold)

    @staticmethod
    def _conv_exec(route, p, extra, device, cmax_in=None, cmax_out=None, cmax_out_relu=False):
        assert (cmax_in is None or route == "wino3h") and (cmax_out is None or route in ("wino3", "wino3h")), route
        if route == "direct":
            check(_L.pf_conv(C.byref(p), _stream()), "pf_conv")
        elif route == "s3_1x1":
            check(_L.pf_conv1x1_split3(C.byref(p), extra[0], extra[1], _stream()), "pf_conv1x1_split3")
        elif route == "fused":
            check(_L.pf_conv_winograd_fused(C.byref(p), extra[0], extra[1], extra[2], _stream()), "pf_conv_winograd_fused")
        elif route == "wino3":
            V, Mw = _workspace(device, extra[3], extra[4])
            if cmax_out is not None:
                check(_L.pf_conv_winograd_split3_windowed_ex(C.byref(p), extra[0], extra[1], extra[2], C.c_void_p(V.data_ptr()), C.c_void_p(Mw.data_ptr()),
                                                             extra[5], C.c_void_p(cmax_out.data_ptr()), int(cmax_out_relu), _stream()),
                      "pf_conv_winograd_split3_windowed_ex")
                return
            check(_L.pf_conv_winograd_split3_windowed(C.byref(p), extra[0], extra[1], extra[2], C.c_void_p(V.data_ptr()), C.c_void_p(Mw.data_ptr()),
                                                      extra[5], _stream()), "pf_conv_winograd_split3_windowed")
        elif route == "wino3h":
            V, Mw = _workspace(device, extra[3], extra[4])
            S = _f16x2_scratch(device, extra[6])
            if cmax_in is not None or cmax_out is not None:
                check(_L.pf_conv_winograd_f16x2_windowed_ex(C.byref(p), extra[0], extra[1], extra[2], C.c_void_p(V.data_ptr()), C.c_void_p(Mw.data_ptr()),
                                                            C.c_void_p(S.data_ptr()), extra[5], None if cmax_in is None else C.c_void_p(cmax_in.data_ptr()),
                                                            None if cmax_out is None else C.c_void_p(cmax_out.data_ptr()), int(cmax_out_relu), _stream()),
                      "pf_conv_winograd_f16x2_windowed_ex")
                return
            check(_L.pf_conv_winograd_f16x2_windowed(C.byref(p), extra[0], extra[1], extra[2], C.c_void_p(V.data_ptr()), C.c_void_p(Mw.data_ptr()),
                                                     C.c_void_p(S.data_ptr()), extra[5], _stream()), "pf_conv_winograd_f16x2_windowed")
        elif route == "wino":
            V, Mw = _workspace(device, extra[4], extra[5])
            check(_L.pf_conv_winograd(C.byref(p), extra[0], extra[1], extra[2], extra[3], C.c_void_p(V.data_ptr()), C.c_void_p(Mw.data_ptr()), _stream()),
                  "pf_conv_winograd")
        else:
            check(_L.pf_gemm_bf16_pp(C.byref(p), _stream()), "pf_gemm_bf16_pp")

    @staticmethod
    def conv(x, pw: PackedConv, y, stride=1, pad=0, act=None, relu_in=False, res=None, res2=None, _timed=None, _direct=None, cmax_in=None):
        """y = epi(conv(x)) through the kernel the dispatch rules pick (pf_conv / fused or three-step Winograd / bf16 ping-pong GEMM).
        The plan of a call -- checks, filled pf_conv_params, route -- is cached per (packed layer, tensor layouts, epilogue); a repeat call only
        refreshes the four data pointers (round-3 review: 22 us of Python per library call, most of it here)."""
        if _timed is None and _direct is None:
            ent = HipOps._conv_plan_cached(x, pw, y, stride, pad, act, relu_in, res, res2, cmax_in is not None)
            if cmax_in is not None and ent[1] != "wino3h":
                raise _lib.PfError("conv: cmax_in given to a layer that does not run the fp16x2 Winograd form (ask cmax_begin first)")
            HipOps._conv_exec(ent[1], ent[2], ent[3], x.device, cmax_in=cmax_in)
            return y
        assert cmax_in is None
        route, p, extra = HipOps._conv_plan(x, pw, y, stride, pad, act, relu_in, res, res2, _direct)
        return HipOps._conv_uncached(route, p, extra, x, y, _timed)

    @staticmethod
    def cmax_begin(x, pw, y, slot, stride=1, pad=0, act=None, relu_in=False, res=None, res2=None):
        """Will conv(x, pw, y, ...) run the fp16x2 Winograd form when the channel maxima of x are handed in?  Then: a zeroed uint32 vector [pw.cin]
        (int32 storage; one memset on the current stream) that the kernels writing x fill slice by slice (resize / resize_concat / roi_align /
        copy_channels with cmax=, absmax for channels another kernel wrote, conv_chain with cmax_out=) and that the conv takes as cmax_in= instead of
        running its range pass.  Else None: write x and call conv as usual.  `slot` names the buffer: vectors alive at the same time need different
        slots.  The maxima are those of the raw stored values, so a consumer with relu_in is refused."""
        if relu_in or not _cmax_handover_enabled() or x.dtype != torch.float32 or x.shape[-1] != pw.cin:
            return None
        ent = HipOps._conv_plan_cached(x, pw, y, stride, pad, act, relu_in, res, res2, True)
        if ent[1] != "wino3h":
            return None
        cm = _cmax_buffer(x.device, pw.cin, slot)[:pw.cin]
        check(_L.pf_zero_u32(_p(cm), pw.cin, _stream()), "pf_zero_u32")
        return cm

    @staticmethod
    def absmax(x, cmax):
        """the range pass alone, on the channels of the NHWC float32 view x: merges max |x[..., c]| (float bits) into cmax[c] (not zeroed here)"""
        x4 = _as4(x)
        B, H, W, Cc = x4.shape
        assert x4.dtype == torch.float32
        check(_L.pf_wino_absmax(_p(x4), _ld(x4), B * H * W, Cc, 0, _cmax_ptr(cmax, Cc), _stream()), "pf_wino_absmax")

    @staticmethod
    def conv_chain(x, pw1, t, pw2, y, kw1, kw2, cmax_in=None, cmax_out=None):
        """t = conv(x, pw1, **kw1); y = conv(t, pw2, **kw2) for a t that conv 2 reads whole and unmodified and nothing else writes (RCU conv1 -> conv2).
        When conv 1 is a three-step Winograd layer and conv 2 an fp16x2 one (by the rule for given maxima), conv 1's output transform hands over the channel
        maxima of t and conv 2 skips its range pass (csrc/wino_f16x2_n256.hip wino_output_cmax_kernel; same bits either way); otherwise exactly two
        conv calls.  cmax_in: the maxima of x from cmax_begin(x, pw1, t, ...).  cmax_out: a uint32 vector [pw2.cout] that receives the maxima of y
        (a slice of the next consumer's vector): from conv 2's output transform when it is a three-step layer, else from the range pass over y."""
        def plan(a, pw, b, kw, given):
            return HipOps._conv_plan_cached(a, pw, b, kw.get("stride", 1), kw.get("pad", 0), kw.get("act"), kw.get("relu_in", False), kw.get("res"),
                                            kw.get("res2"), given)
        e1 = plan(x, pw1, t, kw1, cmax_in is not None)
        if cmax_in is not None and e1[1] != "wino3h":
            raise _lib.PfError("conv_chain: cmax_in given to a layer that does not run the fp16x2 Winograd form (ask cmax_begin first)")
        e2 = None
        if e1[1] in ("wino3", "wino3h") and t.shape[-1] == pw1.cout == pw2.cin and _cmax_handover_enabled():
            e2 = plan(t, pw2, y, kw2, True)
        three = ("wino3", "wino3h")
        if e2 is not None and e2[1] == "wino3h":
            cm = _cmax_buffer(x.device, pw1.cout)
            HipOps._conv_exec(e1[1], e1[2], e1[3], x.device, cmax_in=cmax_in, cmax_out=cm, cmax_out_relu=bool(kw2.get("relu_in", False)))
            HipOps._conv_exec(e2[1], e2[2], e2[3], x.device, cmax_in=cm, cmax_out=cmax_out)
        else:
            e2 = plan(t, pw2, y, kw2, False)
            HipOps._conv_exec(e1[1], e1[2], e1[3], x.device, cmax_in=cmax_in)
            HipOps._conv_exec(e2[1], e2[2], e2[3], x.device, cmax_out=cmax_out if e2[1] in three else None)
            if cmax_out is not None and e2[1] not in three:
                HipOps.absmax(y[..., :pw2.cout], cmax_out)
        return y

    @staticmethod
    def _conv_plan_cached(x, pw, y, stride, pad, act, relu_in, res, res2, given=False):
        key = (id(pw), x.shape, x.stride(), y.shape, y.stride(), stride, pad, act, relu_in, x.dtype, y.dtype, x.device,
               None if res is None else (res.shape, res.stride(), res.dtype), None if res2 is None else (res2.shape, res2.stride(), res2.dtype),
               _align16(x, y, res, res2), bool(given))
        ent = _CONV_CACHE.get(key)
        if ent is None or ent[0] is not pw:
            if len(_CONV_CACHE) > 4096:
                _CONV_CACHE.clear()
            ent = (pw,) + HipOps._conv_plan(x, pw, y, stride, pad, act, relu_in, res, res2, None, given)
            _CONV_CACHE[key] = ent
        else:
            p = ent[2]
            p.x, p.y = x.data_ptr(), y.data_ptr()
            if res is not None:
                p.res = res.data_ptr()
            if res2 is not None:
                p.res2 = res2.data_ptr()
        return ent

    @staticmethod
    def _conv_uncached(route, p, extra, x, y, _timed):
        if _timed is None:
            HipOps._conv_exec(route, p, extra, x.device)
            return y
        if route == "direct":
            ms = C.c_float(0)
            check(_L.pf_conv_timed(C.byref(p), int(_timed), C.byref(ms), _stream()), "pf_conv_timed")
            return ms.value
        if route == "fused":
            ms = C.c_float(0)
            check(_L.pf_conv_winograd_fused_timed(C.byref(p), extra[0], extra[1], extra[2], int(_timed), C.byref(ms), _stream()),
                  "pf_conv_winograd_fused_timed")
            return ms.value
        HipOps._conv_exec(route, p, extra, x.device)          # whole three-step layer / ping-pong GEMM: events on the launch stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(int(_timed)):
            HipOps._conv_exec(route, p, extra, x.device)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / int(_timed)

    @staticmethod
    def gemm_planes_split3(V3, U3, Mw, T, cin, cout, iters=None):
        """the batched split-precision GEMM launch of a three-step Winograd layer alone, exactly as csrc/winograd.hip run_split3 issues it:
        CHUNK-MAJOR operands V3 bf16 [3, P, cin/32, T, 32], U3 bf16 [3, P, cin/32, rows, 32] (PackedConv.wino_u3), Mw float32 [P, T, cout]
        (P = 36 transform points there) -- or both ROW-major, V3 [3, P, T, cin], U3 [3, P, rows, cin] (4-D; tests); iters = None runs it once,
        else returns the average milliseconds of `iters` launches (HIP events on the launch stream; bench.py roofline)"""
        P = V3.shape[1]
        kmaj = V3.dim() == 5
        assert V3.dim() == U3.dim() and V3.dtype == U3.dtype == torch.bfloat16 and Mw.dtype == torch.float32 and U3.shape[:2] == (3, P)
        assert tuple(V3.shape) == ((3, P, cin // 32, T, 32) if kmaj else (3, P, T, cin)) and (U3.shape[2] * 32 if kmaj else U3.shape[3]) == cin
        assert V3.is_contiguous() and U3.is_contiguous() and Mw.is_contiguous() and Mw.numel() >= P * T * cout
        p = ConvParams()
        p.x, p.x_ld, p.B, p.H, p.W, p.Cin = V3.data_ptr(), cin, 1, 1, T, cin
        p.w, p.w_rows, p.Kpad = U3.data_ptr(), U3.shape[3] if kmaj else U3.shape[2], cin
        p.korder = 6 if kmaj else 0
        p.y, p.y_ld, p.OH, p.OW, p.Cout = Mw.data_ptr(), cout, 1, T, cout
        p.KH = p.KW = p.stride = 1
        p.act, p.shuffle, p.dtype, p.out_f32, p.batch = 0, 1, 1, 1, P
        p.x_bstride, p.w_bstride = V3.stride(0), U3.stride(0)
        for t in (V3, U3, Mw):
            _p(t)
        if iters is None:
            check(_L.pf_gemm_split3(C.byref(p), _stream()), "pf_gemm_split3")
            return Mw
        ms = C.c_float(0)
        check(_L.pf_gemm_split3_timed(C.byref(p), int(iters), C.byref(ms), _stream()), "pf_gemm_split3_timed")
        return ms.value

    @staticmethod
    def gemm_planes_split3_timed(V3, U3, Mw, T, cin, cout, iters):
        return HipOps.gemm_planes_split3(V3, U3, Mw, T, cin, cout, iters)

    @staticmethod
    def gemm_planes_timed(V, U, Mw, planes, T, cin, cout, iters):
        """time the batched GEMM launch of a Winograd layer alone (bench.py roofline): `planes` x ([T, cin] . [cout, cin]^T) through
        pf_conv with pf_conv_params.batch, exactly as csrc/winograd.hip issues it; V / Mw float32 workspaces, U [planes, rows, Kpad]"""
        assert V.dtype == U.dtype == Mw.dtype == torch.float32 and V.numel() >= planes * T * cin and Mw.numel() >= planes * T * cout
        p = ConvParams()
        p.x, p.x_ld, p.B, p.H, p.W, p.Cin = V.data_ptr(), cin, 1, 1, T, cin
        p.w, p.w_rows, p.Kpad = U.data_ptr(), U.shape[1], U.shape[2]
        p.y, p.y_ld, p.OH, p.OW, p.Cout = Mw.data_ptr(), cout, 1, T, cout
        p.KH = p.KW = p.stride = 1
        p.shuffle, p.dtype = 1, 0
        p.batch, p.x_bstride, p.w_bstride, p.y_bstride = planes, T * cin, U.shape[1] * U.shape[2], T * cout
        for t in (V, U, Mw):
            _p(t)
        ms = C.c_float(0)
        check(_L.pf_conv_timed(C.byref(p), int(iters), C.byref(ms), _stream()), "pf_conv_timed")
        return ms.value

    # ---------------- split-precision GEMM (exploratory "f32x3" mode) ----------------
    @staticmethod
    def split3(x, y3):
        """x float32 [M, K] (row stride >= K) -> y3 bfloat16 [3, M, K] planes"""
        assert x.dtype == torch.float32 and y3.dtype == torch.bfloat16 and y3.dim() == 3 and y3.shape[0] == 3 and y3.is_contiguous()
        M, K = x.shape
        check(_L.pf_split3(_p(x), x.stride(0), _p(y3), y3.stride(1), y3.stride(0), M, K, _stream()), "pf_split3")
        return y3

    @staticmethod
    def _conv_split3_plan(x3, pw, y, act, res, res2):
        """x3 bfloat16 [3, M, K] planes; pw from packing.pack_conv_split3; y float32 [M, N] or bfloat16 [3, M, N] planes (split output);
        res / res2 float32 [M, N].  float32-grade linear layer on the bf16 matrix cores (csrc/gemm_split3.hip)."""
        assert x3.dtype == torch.bfloat16 and x3.shape[0] == 3 and pw.w.dtype == torch.bfloat16
        split_out = y.dtype == torch.bfloat16
        p = ConvParams()
        korder = 0
        if x3.dim() == 4:                                     # chunk-major planes [3, K/32, M, 32]
            assert x3.is_contiguous() and x3.shape[3] == 32 and x3.shape[1] * 32 == pw.cin
            M = x3.shape[2]
            p.x, p.x_ld = x3.data_ptr(), pw.cin
            korder |= 2
        else:
            assert x3.dim() == 3 and x3.stride(2) == 1 and x3.shape[2] >= pw.cin
            M = x3.shape[1]
            p.x, p.x_ld = x3.data_ptr(), x3.stride(1)
        p.B, p.H, p.W, p.Cin = 1, 1, M, pw.cin
        p.x_bstride = x3.stride(0)
        if pw.w.dim() == 4:                                   # chunk-major weight planes [3, K/32, rows, 32] (packing.pack_conv_split3)
            assert pw.w.is_contiguous() and pw.w.shape[1] * 32 == pw.cin
            p.w, p.w_rows, p.Kpad, p.w_bstride = pw.w.data_ptr(), pw.w.shape[2], pw.cin, pw.w.stride(0)
            korder |= 4
        else:
            p.w, p.w_rows, p.Kpad, p.w_bstride = pw.w.data_ptr(), pw.w.shape[1], pw.w.shape[2], pw.w.stride(0)
        p.bias = pw.bias.data_ptr() if pw.bias is not None else None
        p.scale = pw.scale.data_ptr() if pw.scale is not None else None
        p.res = res.data_ptr() if res is not None else None
        p.res_ld = res.stride(-2) if res is not None else 0
        p.res2 = res2.data_ptr() if res2 is not None else None
        p.res2_ld = res2.stride(-2) if res2 is not None else 0
        if split_out and y.dim() == 4:                        # chunk-major output planes [3, N/32, M, 32]
            assert y.is_contiguous() and tuple(y.shape) == (3, pw.cout // 32, M, 32) and pw.cout % 32 == 0
            p.y, p.y_ld, p.y_bstride, p.out_f32 = y.data_ptr(), pw.cout, y.stride(0), 0
            korder |= 8
        elif split_out:
            assert y.dim() == 3 and y.shape[0] == 3 and y.shape[1] == M and y.stride(2) == 1
            p.y, p.y_ld, p.y_bstride, p.out_f32 = y.data_ptr(), y.stride(1), y.stride(0), 0
        else:
            assert y.dtype == torch.float32 and y.stride(-1) == 1
            p.y, p.y_ld, p.out_f32 = y.data_ptr(), y.stride(-2), 1
        p.OH, p.OW, p.Cout = 1, M, pw.cout
        p.KH = p.KW = p.stride = 1
        p.act, p.shuffle, p.dtype, p.korder = ACT[act], 1, 1, korder
        for t in (x3, y, pw.w, res, res2):
            _p(t)                                             # (device / layout checks of every tensor handed to the library)
        for t in (res, res2):
            assert t is None or (t.dtype == torch.float32 and t.shape[-1] >= pw.cout and t.shape[-2] == M), "residuals are float32 [M, >= N]"
        assert y.dim() == 4 or (y.shape[-1] >= pw.cout and y.shape[-2] == M)
        return p

    @staticmethod
    def conv_split3(x3, pw: PackedConv, y, act=None, res=None, res2=None, _timed=None):
        """x3 bfloat16 planes, row-major [3, M, K] or chunk-major [3, K/32, M, 32]; pw from packing.pack_conv_split3; y float32 [M, N] or bfloat16
        planes ([3, M, N] / chunk-major [3, N/32, M, 32]: split output for a following split GEMM); res / res2 float32 [M, N].  float32-grade linear
        layer on the bf16 matrix cores (csrc/gemm_split3.hip).  Like HipOps.conv, the checked and filled pf_conv_params of a call is cached per
        (layer, layouts); a repeat call refreshes the data pointers only."""
        key = (id(pw), x3.shape, x3.stride(), y.shape, y.stride(), y.dtype, act, x3.device,
               None if res is None else (res.shape, res.stride()), None if res2 is None else (res2.shape, res2.stride()))
        ent = _CONV_CACHE.get(key)
        if ent is None or ent[0] is not pw:
            if len(_CONV_CACHE) > 4096:
                _CONV_CACHE.clear()
            ent = (pw, HipOps._conv_split3_plan(x3, pw, y, act, res, res2))
            _CONV_CACHE[key] = ent
        else:
            p = ent[1]
            p.x, p.y = x3.data_ptr(), y.data_ptr()
            if res is not None:
                p.res = res.data_ptr()
            if res2 is not None:
                p.res2 = res2.data_ptr()
        p = ent[1]
        if _timed is not None:
            ms = C.c_float(0)
            check(_L.pf_gemm_split3_timed(C.byref(p), int(_timed), C.byref(ms), _stream()), "pf_gemm_split3_timed")
            return ms.value
        check(_L.pf_gemm_split3(C.byref(p), _stream()), "pf_gemm_split3")
        return y

    @staticmethod
    def _conv_f16x2_plan(x2, pw, y, act, res, res2, out_exp):
        assert x2.dtype == pw.w.dtype == torch.float16 and x2.dim() == 4 and x2.shape[0] == 2 and x2.shape[3] == 32 and x2.is_contiguous()
        assert x2.shape[1] * 32 == pw.cin and pw.w.dim() == 4 and pw.w.is_contiguous() and pw.col_exp is not None
        M = x2.shape[2]
        p = ConvParams()
        p.x, p.x_ld, p.x_bstride = x2.data_ptr(), pw.cin, x2.stride(0)
        p.B, p.H, p.W, p.Cin = 1, 1, M, pw.cin
        p.w, p.w_rows, p.Kpad, p.w_bstride = pw.w.data_ptr(), pw.w.shape[2], pw.cin, pw.w.stride(0)
        p.bias = pw.bias.data_ptr() if pw.bias is not None else None
        p.scale = pw.scale.data_ptr() if pw.scale is not None else None
        p.col_exp = _p(pw.col_exp)
        p.res = res.data_ptr() if res is not None else None
        p.res_ld = res.stride(-2) if res is not None else 0
        p.res2 = res2.data_ptr() if res2 is not None else None
        p.res2_ld = res2.stride(-2) if res2 is not None else 0
        korder = 6
        if y.dtype == torch.float16 and y.dim() == 3:         # fp16x2 planes of y / 2^out_exp, row-major [2, M, N] (q / k / v of the fp16x2 attention)
            assert y.shape[0] == 2 and y.shape[1] == M and y.stride(2) == 1 and y.shape[2] >= pw.cout and y.stride(1) % 4 == 0
            assert out_exp is not None and out_exp.dtype == torch.int32 and out_exp.numel() >= pw.cout
            p.y, p.y_ld, p.y_bstride, p.out_f32, p.out_exp = y.data_ptr(), y.stride(1), y.stride(0), 0, _p(out_exp)
            korder |= 32
        elif y.dtype == torch.float16:                        # fp16x2 planes of y / 2^out_exp for the next fp16x2 linear, chunk-major [2, N/32, M, 32]
            assert y.is_contiguous() and tuple(y.shape) == (2, pw.cout // 32, M, 32) and pw.cout % 32 == 0
            assert out_exp is not None and out_exp.dtype == torch.int32 and out_exp.numel() >= pw.cout
            p.y, p.y_ld, p.y_bstride, p.out_f32, p.out_exp = y.data_ptr(), pw.cout, y.stride(0), 0, _p(out_exp)
            korder |= 16
        elif y.dtype == torch.bfloat16:                       # three bf16 planes, row-major [3, M, N] (the attention's q / k / v)
            assert y.dim() == 3 and y.shape[0] == 3 and y.shape[1] == M and y.stride(2) == 1 and y.shape[2] >= pw.cout
            p.y, p.y_ld, p.y_bstride, p.out_f32 = y.data_ptr(), y.stride(1), y.stride(0), 0
        else:
            assert y.dtype == torch.float32 and y.stride(-1) == 1 and y.shape[-2] == M and y.shape[-1] >= pw.cout
            p.y, p.y_ld, p.out_f32 = y.data_ptr(), y.stride(-2), 1
        p.OH, p.OW, p.Cout = 1, M, pw.cout
        p.KH = p.KW = p.stride = 1
        p.act, p.shuffle, p.dtype, p.korder = ACT[act], 1, 1, korder
        for t in (x2, y, pw.w, res, res2):
            _p(t)
        for t in (res, res2):
            assert t is None or (t.dtype == torch.float32 and t.shape[-1] >= pw.cout and t.shape[-2] == M), "residuals are float32 [M, >= N]"
        return p

    @staticmethod
    def conv_f16x2(x2, pw: PackedConv, y, act=None, res=None, res2=None, out_exp=None):
        """x2 float16 planes [2, K/32, M, 32] holding x / 2^pw.in_exp (ops.layernorm_f16x2 or a previous conv_f16x2); pw from packing.pack_conv_f16x2;
        y float32 [M, N], bfloat16 [3, M, N] (three split planes, row-major), float16 [2, N/32, M, 32] (planes of y / 2^out_exp for the next
        fp16x2 linear) or float16 [2, M, N] (the same planes row-major: q / k / v of ops.vit_attention_f16x2); res / res2 float32 [M, N].  csrc/gemm_split3.hip pf_gemm_f16x2; plans cached like conv_split3."""
        key = ("f16x2", id(pw), x2.shape, y.shape, y.stride(), y.dtype, act, x2.device,
               None if res is None else (res.shape, res.stride()), None if res2 is None else (res2.shape, res2.stride()),
               None if out_exp is None else out_exp.data_ptr())
        ent = _CONV_CACHE.get(key)
        if ent is None or ent[0] is not pw:
            if len(_CONV_CACHE) > 4096:
                _CONV_CACHE.clear()
            ent = (pw, HipOps._conv_f16x2_plan(x2, pw, y, act, res, res2, out_exp))
            _CONV_CACHE[key] = ent
        else:
            p = ent[1]
            p.x, p.y = x2.data_ptr(), y.data_ptr()
            if res is not None:
                p.res = res.data_ptr()
            if res2 is not None:
                p.res2 = res2.data_ptr()
        check(_L.pf_gemm_f16x2(C.byref(ent[1]), _stream()), "pf_gemm_f16x2")
        return y

    # ---------------- ViT ----------------
    @staticmethod
    def patch_im2col(img, out):
        B, _, H, W = img.shape
        assert img.dtype == torch.float32 and img.is_contiguous()
        check(_L.pf_patch_im2col(_p(img), B, H, W, _p(out), out.stride(0), _dt(out), _stream()), "pf_patch_im2col")

    @staticmethod
    def assemble_tokens(emb, tokens, cls, pos):
        B, S, D = tokens.shape
        assert emb.is_contiguous() and tokens.is_contiguous()
        check(_L.pf_assemble_tokens(_p(emb), _p(tokens), _p(cls), _p(pos), B, S, D, _dt(tokens), _stream()), "pf_assemble_tokens")

    @staticmethod
    def layernorm(x, y, g, b, eps, batches=1, in_rows_per_batch=None, in_row_offset=0, out_rows_per_batch=None):
        D = x.shape[-1]
        rows = x.numel() // D
        if in_rows_per_batch is None:
            in_rows_per_batch = out_rows_per_batch = rows
            batches = 1
        check(_L.pf_layernorm(_p(x), x.stride(-2), _p(y), y.stride(-2), _p(g), _p(b), float(eps), batches, in_rows_per_batch,
                              in_row_offset, out_rows_per_batch, D, _dt(x), _stream()), "pf_layernorm")

    @staticmethod
    def layernorm_split3(x, y3, g, b, eps):
        """LayerNorm of float32 rows x [M, D], output as three bfloat16 planes (input of ops.conv_split3): y3 [3, M, D] row-major or
        [3, D/32, M, 32] chunk-major"""
        assert x.dtype == torch.float32 and y3.dtype == torch.bfloat16 and y3.shape[0] == 3
        M, D = x.shape
        if y3.dim() == 4:
            assert y3.is_contiguous() and tuple(y3.shape) == (3, D // 32, M, 32)
            check(_L.pf_layernorm_split3(_p(x), x.stride(0), _p(y3), D, y3.stride(0), 1, _p(g), _p(b), float(eps), M, D, _stream()),
                  "pf_layernorm_split3")
            return y3
        assert y3.dim() == 3 and y3.stride(2) == 1 and y3.shape[1] == M and y3.shape[2] == D
        check(_L.pf_layernorm_split3(_p(x), x.stride(0), _p(y3), y3.stride(1), y3.stride(0), 0, _p(g), _p(b), float(eps), M, D, _stream()),
              "pf_layernorm_split3")
        return y3

    @staticmethod
    def layernorm_f16x2(x, y2, g, b, eps, in_exp):
        """LayerNorm of float32 rows x [M, D] as the fp16x2 input of ops.conv_f16x2: y2 float16 [2, D/32, M, 32] = LN(x) / 2^in_exp split h + l"""
        assert x.dtype == torch.float32 and x.stride(-1) == 1 and y2.dtype == torch.float16 and in_exp.dtype == torch.int32
        M, D = x.shape
        assert y2.is_contiguous() and tuple(y2.shape) == (2, D // 32, M, 32) and in_exp.numel() == D
        check(_L.pf_layernorm_f16x2(_p(x), x.stride(0), _p(y2), _p(in_exp), _p(g), _p(b), float(eps), M, D, _stream()), "pf_layernorm_f16x2")
        return y2

    @staticmethod
    def vit_attention(qkv, out, B, S, heads):
        """qkv [B*S, 3*D] -> out [B*S, D]; head_dim must be 64.  float32 qkv with a bfloat16 out [3, B*S, D]: the output is written as
        the three split planes of the projection GEMM (ops.conv_split3)."""
        kmaj = int(out.dim() == 4)                            # output planes chunk-major [3, D/32, B*S, 32] (input of the projection GEMM)
        if qkv.dim() == 3:
            # the QKV GEMM's output as three bf16 planes [3, B*S, 3*D]: attention entirely in split precision (csrc/vit.hip)
            D = qkv.shape[2] // 3
            assert qkv.dtype == out.dtype == torch.bfloat16 and tuple(qkv.shape) == (3, B * S, 3 * D)
            assert tuple(out.shape) == ((3, D // 32, B * S, 32) if kmaj else (3, B * S, D))
            assert D == heads * 64 and qkv.is_contiguous() and out.is_contiguous()
            # PF_ATTN_V2 (default 1): csrc/attn_split3.hip (LDS-DMA tiles, transposing V reads); PF_ATTN_QW = 16 / 32 forces the queries per wave
            # (0: by launch size), PF_ATTN_SCHED = 1 the two-phase kernel (bit-identical to version 1) / 2 the software-pipelined kernel (0: default)
            if _env("PF_ATTN_V2", "1") != "0":
                check(_L.pf_vit_attention_split3_v2(_p(qkv), qkv.stride(0), _p(out), out.stride(0), kmaj, B, S, heads, int(_env("PF_ATTN_QW", "0")),
                                                    int(_env("PF_ATTN_SCHED", "0")), _stream()), "pf_vit_attention_split3_v2")
                return
            check(_L.pf_vit_attention_split3(_p(qkv), qkv.stride(0), _p(out), out.stride(0), kmaj, B, S, heads, _stream()), "pf_vit_attention_split3")
            return
        D = qkv.shape[1] // 3
        assert D == heads * 64 and qkv.is_contiguous() and out.is_contiguous()
        if qkv.dtype == torch.float32 and out.dtype == torch.bfloat16:
            assert tuple(out.shape) == ((3, D // 32, B * S, 32) if kmaj else (3, B * S, D))
            check(_L.pf_vit_attention_qkv_split3(_p(qkv), _p(out), out.stride(0), kmaj, B, S, heads, _stream()), "pf_vit_attention_qkv_split3")
            return
        if qkv.dtype == torch.float32 and _env("PF_ATTN_QKV", "1") != "0":
            # f32: the attention kernel reads q / k / v rows straight out of the QKV GEMM's output (csrc/vit.hip, version 2)
            check(_L.pf_vit_attention_qkv(_p(qkv), _p(out), B, S, heads, 0, _stream()), "pf_vit_attention_qkv")
            return
        Sp = (S + 63) // 64 * 64
        q = torch.empty((B, heads, S, 64), dtype=qkv.dtype, device=qkv.device)
        k = torch.empty_like(q)
        vt = torch.empty((B, heads, 64, Sp), dtype=qkv.dtype, device=qkv.device)
        check(_L.pf_qkv_split(_p(qkv), B, S, heads, _p(q), _p(k), _p(vt), Sp, 0.125, _dt(qkv), _stream()), "pf_qkv_split")
        check(_L.pf_vit_attention(_p(q), _p(k), _p(vt), _p(out), B, S, Sp, heads, _dt(qkv), _stream()), "pf_vit_attention")

    @staticmethod
    def vit_attention_f16x2(qkv2, out2, B, S, heads, qk_exp, v_exp=None):
        """ViT attention on two scaled fp16 planes (csrc/attn_split3.hip pf_vit_attention_f16x2): qkv2 float16 [2, B*S, 3*D] from ops.conv_f16x2 with the
        exponents of packing.vit_attn_f16x2_scales, qk_exp int32 [heads] on the device; out2 float16 [2, D/32, B*S, 32], the projection's fp16x2 input
        (out / 2^ev), or -- with v_exp = ev int32 [D] -- bfloat16 [3, D/32, B*S, 32], the three split planes of the output for ops.conv_split3."""
        D = heads * 64
        if v_exp is not None:
            if out2.dtype != torch.bfloat16 or tuple(out2.shape) != (3, D // 32, B * S, 32) or not out2.is_contiguous():
                raise ValueError(f"vit_attention_f16x2: bad bf16x3 output planes {out2.dtype} {tuple(out2.shape)}")
            if v_exp.dtype != torch.int32 or v_exp.numel() != D or not v_exp.is_contiguous() or v_exp.device != qkv2.device:
                raise ValueError(f"vit_attention_f16x2: v_exp must be contiguous int32 [{D}] on {qkv2.device}")
        if qkv2.dtype != torch.float16 or tuple(qkv2.shape) != (2, B * S, 3 * D) or not qkv2.is_contiguous():
            raise ValueError(f"vit_attention_f16x2: qkv2 must be contiguous float16 [2, {B * S}, {3 * D}], got {qkv2.dtype} {tuple(qkv2.shape)}")
        if v_exp is None and (out2.dtype != torch.float16 or tuple(out2.shape) != (2, D // 32, B * S, 32) or not out2.is_contiguous()):
            raise ValueError(f"vit_attention_f16x2: bad output planes {out2.dtype} {tuple(out2.shape)}")
        if qk_exp.dtype != torch.int32 or qk_exp.numel() != heads or not qk_exp.is_contiguous() or qk_exp.device != qkv2.device:
            raise ValueError(f"vit_attention_f16x2: qk_exp must be contiguous int32 [{heads}] on {qkv2.device}")
        check(_L.pf_vit_attention_f16x2(_p(qkv2), qkv2.stride(0), _p(qk_exp), _p(out2), out2.stride(0), None if v_exp is None else _p(v_exp), B, S, heads,
                                        _stream()), "pf_vit_attention_f16x2")

    @staticmethod
    def vit_attention_rpb(qkv, out, B, S, heads, tab, th, tw):
        """BEiT attention with a per-head relative-position bias (MiDaS DPT_BEiT_L_384 core, csrc/attn_split3.hip pf_vit_attention_split3_rpb):
        qkv bfloat16 [3, B*S, 3*D] planes of the QKV GEMM -> out bfloat16 [3, B*S, D] (or chunk-major [3, D/32, B*S, 32]) planes; tab float32
        [heads, (2 th - 1)(2 tw - 1) + 3] on the device, interpolated to (th, tw) and multiplied by log2(e) (packing.beit_rel_pos_tables)."""
        kmaj = int(out.dim() == 4)
        D = heads * 64
        if qkv.dtype != torch.bfloat16 or tuple(qkv.shape) != (3, B * S, 3 * D) or not qkv.is_contiguous():
            raise ValueError(f"vit_attention_rpb: qkv must be contiguous bfloat16 [3, {B * S}, {3 * D}], got {qkv.dtype} {tuple(qkv.shape)}")
        if out.dtype != torch.bfloat16 or tuple(out.shape) != ((3, D // 32, B * S, 32) if kmaj else (3, B * S, D)) or not out.is_contiguous():
            raise ValueError(f"vit_attention_rpb: bad output planes {out.dtype} {tuple(out.shape)}")
        if S != th * tw + 1:
            raise ValueError(f"vit_attention_rpb: S = {S} is not th * tw + 1 = {th * tw + 1}")
        ntab = (2 * th - 1) * (2 * tw - 1) + 3
        if tab.dtype != torch.float32 or tuple(tab.shape) != (heads, ntab) or not tab.is_contiguous() or tab.device != qkv.device:
            raise ValueError(f"vit_attention_rpb: tab must be contiguous float32 [{heads}, {ntab}] on {qkv.device}")
        check(_L.pf_vit_attention_split3_rpb(_p(qkv), qkv.stride(0), _p(out), out.stride(0), kmaj, B, S, heads, _p(tab), th, tw,
                                             int(_env("PF_ATTN_QW", "0")), _stream()), "pf_vit_attention_split3_rpb")

    @staticmethod
    def vit_attention_rpb_bf16(qkv, out, B, S, heads, tab, th, tw):
        """The same BEiT attention in the bf16 mode (csrc/vit.hip pf_vit_attention_rpb_bf16): qkv bfloat16 [B*S, 3*D] rows of the QKV GEMM -> out
        bfloat16 [B*S, D]; pf_qkv_split (q scaled by head_dim^-1/2, rounded to bf16) + the biased 32-queries-per-wave kernel.  tab float32 as above."""
        D = heads * 64
        if qkv.dtype != torch.bfloat16 or tuple(qkv.shape) != (B * S, 3 * D) or not qkv.is_contiguous():
            raise ValueError(f"vit_attention_rpb_bf16: qkv must be contiguous bfloat16 [{B * S}, {3 * D}], got {qkv.dtype} {tuple(qkv.shape)}")
        if out.dtype != torch.bfloat16 or tuple(out.shape) != (B * S, D) or not out.is_contiguous() or out.device != qkv.device:
            raise ValueError(f"vit_attention_rpb_bf16: out must be contiguous bfloat16 [{B * S}, {D}] on {qkv.device}, got {out.dtype} {tuple(out.shape)}")
        if S != th * tw + 1 or tw < 4:
            raise ValueError(f"vit_attention_rpb_bf16: S = {S} must be th * tw + 1 = {th * tw + 1} with tw >= 4")
        ntab = (2 * th - 1) * (2 * tw - 1) + 3
        if tab.dtype != torch.float32 or tuple(tab.shape) != (heads, ntab) or not tab.is_contiguous() or tab.device != qkv.device:
            raise ValueError(f"vit_attention_rpb_bf16: tab must be contiguous float32 [{heads}, {ntab}] on {qkv.device}")
        Sp = (S + 63) // 64 * 64
        q = torch.empty((B, heads, S, 64), dtype=qkv.dtype, device=qkv.device)
        k = torch.empty_like(q)
        vt = torch.empty((B, heads, 64, Sp), dtype=qkv.dtype, device=qkv.device)
        check(_L.pf_qkv_split(_p(qkv), B, S, heads, _p(q), _p(k), _p(vt), Sp, 0.125, 1, _stream()), "pf_qkv_split")
        check(_L.pf_vit_attention_rpb_bf16(_p(q), _p(k), _p(vt), _p(out), B, S, Sp, heads, _p(tab), th, tw, _stream()), "pf_vit_attention_rpb_bf16")

    @staticmethod
    def patch_im2col_norm(img, out, patch, mean, std):
        """img float32 [B,3,H,W] -> out float32 (or bfloat16: the bf16 mode, rounded once) [B*(H/patch)*(W/patch), ld >= 3 patch^2] rows of
        (x - mean[c]) / std[c] (K order ky, kx, c)"""
        B, Ci, H, W = img.shape
        if img.dtype != torch.float32 or not img.is_contiguous() or Ci != 3 or H % patch or W % patch:
            raise ValueError(f"patch_im2col_norm: img must be contiguous float32 [B,3,H,W] with H, W multiples of {patch}")
        if out.dtype == torch.bfloat16:
            if out.dim() != 2 or out.shape[0] != B * (H // patch) * (W // patch) or out.shape[1] < 3 * patch * patch or out.stride(1) != 1 \
                    or out.device != img.device:
                raise ValueError(f"patch_im2col_norm: bad output {out.dtype} {tuple(out.shape)}")
            m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
            check(_L.pf_patch_im2col_norm_bf16(_p(img), B, H, W, patch, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), _p(out), out.stride(0),
                                               _stream()), "pf_patch_im2col_norm_bf16")
            return
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B * (H // patch) * (W // patch) or out.shape[1] < 3 * patch * patch \
                or out.stride(1) != 1:
            raise ValueError(f"patch_im2col_norm: bad output {out.dtype} {tuple(out.shape)}")
        m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
        check(_L.pf_patch_im2col_norm(_p(img), B, H, W, patch, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), _p(out), out.stride(0), _stream()),
              "pf_patch_im2col_norm")

    @staticmethod
    def readout_concat(x, y, B, S):
        """x float32 [B*S, D] token rows (row stride >= D) -> y float32 [B*(S-1), 2D] rows [token | cls of its image]; both bfloat16 in the bf16 mode"""
        D = x.shape[1]
        if x.dtype == torch.bfloat16:
            if y.dtype != torch.bfloat16 or x.shape[0] != B * S or x.stride(1) != 1 or y.stride(1) != 1 or x.device != y.device:
                raise ValueError("readout_concat: bfloat16 row-major operands on one device required")
            if tuple(y.shape) != (B * (S - 1), 2 * D) or D % 8 or x.stride(0) % 8 or y.stride(0) % 8 or (x.data_ptr() | y.data_ptr()) & 15:
                raise ValueError(f"readout_concat: bad shapes / strides / alignment x {tuple(x.shape)} y {tuple(y.shape)}")
            check(_L.pf_readout_concat_bf16(_p(x), x.stride(0), B, S, D, _p(y), y.stride(0), _stream()), "pf_readout_concat_bf16")
            return
        if x.dtype != torch.float32 or y.dtype != torch.float32 or x.shape[0] != B * S or x.stride(1) != 1 or y.stride(1) != 1:
            raise ValueError("readout_concat: float32 row-major operands required")
        if tuple(y.shape) != (B * (S - 1), 2 * D) or D % 4 or x.stride(0) % 4 or y.stride(0) % 4 or (x.data_ptr() | y.data_ptr()) & 15:
            raise ValueError(f"readout_concat: bad shapes / strides / alignment x {tuple(x.shape)} y {tuple(y.shape)}")
        check(_L.pf_readout_concat(_p(x), x.stride(0), B, S, D, _p(y), y.stride(0), _stream()), "pf_readout_concat")

    # ---------------- Swin / G2L ----------------
    @staticmethod
    def swin_ln_partition(x, xw, g, b, eps, shift):
        B, H, W, Cc = x.shape
        assert xw.is_contiguous()
        check(_L.pf_swin_ln_partition(_p(x), _ld(x), _p(xw), _p(g), _p(b), float(eps), B, H, W, Cc, shift, _dt(x), _stream()),
              "pf_swin_ln_partition")

    @staticmethod
    def swin_window_attention(qkv, out, bias_table, B, Hp, Wp, Cc, heads, shift):
        assert qkv.is_contiguous() and out.is_contiguous() and bias_table.is_contiguous()
        check(_L.pf_swin_window_attention(_p(qkv), _p(out), _p(bias_table), B, Hp, Wp, Cc, heads, shift, _dt(qkv), _stream()),
              "pf_swin_window_attention")

    @staticmethod
    def swin_unpartition_add(proj, shortcut, y, shift):
        B, H, W, Cc = shortcut.shape
        check(_L.pf_swin_unpartition_add(_p(proj), _p(shortcut), _ld(shortcut), _p(y), _ld(y), B, H, W, Cc, shift, _dt(y), _stream()),
              "pf_swin_unpartition_add")

    @staticmethod
    def add_rowwise(x, pos):
        """x [B,T,C] += pos [T,C] (float32)"""
        B, T, Cc = x.shape
        check(_L.pf_add_rowwise(_p(x), x.stride(1), _p(pos), B, T, Cc, _dt(x), _stream()), "pf_add_rowwise")

    # ---------------- image ops ----------------
    @staticmethod
    def resize(x, y, add=None, dtype=None, cmax=None):
        """cmax (float32 calls): a uint32 vector [C] into which the kernel merges the channel maxima of what it stores (HipOps.cmax_begin)"""
        x4, y4 = _as4(x), _as4(y)
        B, H, W, Cc = x4.shape
        _, OH, OW, _ = y4.shape
        cd = dtype if dtype is not None else (x4.dtype if x4.dtype != torch.float32 else y4.dtype)
        code = 1 if cd == torch.bfloat16 else 0
        in_f32 = int(x4.dtype == torch.float32)
        out_f32 = int(y4.dtype == torch.float32)
        if add is not None:
            assert add.dtype == y4.dtype
        if cmax is not None:
            check(_L.pf_resize_bilinear_ex(_p(x4), _ld(x4), B, H, W, Cc, _p(y4), _ld(y4), OH, OW, _p(add), _ld(add) if add is not None else 0,
                                           in_f32, out_f32, code, _cmax_ptr(cmax, Cc), _stream()), "pf_resize_bilinear_ex")
            return
        check(_L.pf_resize_bilinear(_p(x4), _ld(x4), B, H, W, Cc, _p(y4), _ld(y4), OH, OW, _p(add), _ld(add) if add is not None else 0,
                                    in_f32, out_f32, code, _stream()), "pf_resize_bilinear")

    @staticmethod
    def resize_concat(xs, y, cmax=None):
        """y[..., c0:c0+C_i] = bilinear(xs[i]) for 2 or 3 NHWC sources of the compute dtype (one launch, whole rows of y); cmax: as HipOps.resize,
        indexed like the channels of y"""
        n = len(xs)
        y4 = _as4(y)
        B, OH, OW, Ct = y4.shape
        assert 2 <= n <= 3 and sum(x.shape[-1] for x in xs) <= Ct and all(x.dtype == y4.dtype and x.shape[0] == B for x in xs)
        ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
        arr = lambda v: (C.c_int * n)(*v)
        for t in list(xs) + [y4]:
            _p(t)
        if cmax is not None:
            check(_L.pf_resize_concat_ex(ptrs, arr([_ld(x) for x in xs]), arr([x.shape[1] for x in xs]), arr([x.shape[2] for x in xs]),
                                         arr([x.shape[3] for x in xs]), n, B, _p(y4), _ld(y4), OH, OW, _dt(y4),
                                         _cmax_ptr(cmax, sum(x.shape[3] for x in xs)), _stream()), "pf_resize_concat_ex")
            return
        check(_L.pf_resize_concat(ptrs, arr([_ld(x) for x in xs]), arr([x.shape[1] for x in xs]), arr([x.shape[2] for x in xs]),
                                  arr([x.shape[3] for x in xs]), n, B, _p(y4), _ld(y4), OH, OW, _dt(y4), _stream()), "pf_resize_concat")

    @staticmethod
    def crop_resize(img, boxes, out):
        """img [3,H,W] f32; boxes int32 [P,4] (x0,y0,x1,y1) on device; out [P,3,oh,ow] f32"""
        Cc, H, W = img.shape
        P, _, oh, ow = out.shape
        assert img.is_contiguous() and out.is_contiguous() and boxes.dtype == torch.int32
        check(_L.pf_crop_resize_planar(_p(img), Cc, H, W, _p(boxes), P, _p(out), oh, ow, _stream()), "pf_crop_resize_planar")

    @staticmethod
    def roi_align_depth(feat, rois, y, spatial_scale):
        """single-channel planar float map: feat [Bf,1,H,W] f32 -> y [K,1,oh,ow] f32"""
        Bf, _, H, W = feat.shape
        K, _, oh, ow = y.shape
        assert feat.is_contiguous() and y.is_contiguous() and feat.dtype == y.dtype == torch.float32
        check(_L.pf_roi_align(_p(feat), 1, Bf, H, W, 1, _p(rois), K, _p(y), 1, oh, ow, float(spatial_scale), 1, 1, 0, _stream()),
              "pf_roi_align")

    @staticmethod
    def roi_align(feat, rois, y, spatial_scale, dtype=None, cmax=None):
        """feat [Bf,H,W,C] NHWC; rois f32 [K,5]; y [K,oh,ow,C]; cmax: as HipOps.resize"""
        Bf, H, W, Cc = feat.shape
        K, oh, ow, _ = y.shape
        code = 1 if (dtype or feat.dtype) == torch.bfloat16 else 0
        if cmax is not None:
            check(_L.pf_roi_align_ex(_p(feat), _ld(feat), Bf, H, W, Cc, _p(rois), K, _p(y), _ld(y), oh, ow, float(spatial_scale),
                                     int(feat.dtype == torch.float32), int(y.dtype == torch.float32), code, _cmax_ptr(cmax, Cc), _stream()),
                  "pf_roi_align_ex")
            return
        check(_L.pf_roi_align(_p(feat), _ld(feat), Bf, H, W, Cc, _p(rois), K, _p(y), _ld(y), oh, ow, float(spatial_scale),
                              int(feat.dtype == torch.float32), int(y.dtype == torch.float32), code, _stream()), "pf_roi_align")

    @staticmethod
    def maxpool2(x, y):
        B, H, W, Cc = x.shape
        check(_L.pf_maxpool2(_p(x), _ld(x), B, H, W, Cc, _p(y), _ld(y), _dt(x), _stream()), "pf_maxpool2")

    @staticmethod
    def copy_channels(x, y, cmax=None):
        """cmax: as HipOps.resize"""
        x4, y4 = _as4(x), _as4(y)
        B, H, W, Cc = x4.shape
        code = 1 if torch.bfloat16 in (x4.dtype, y4.dtype) else 0
        if cmax is not None:
            check(_L.pf_copy_channels_ex(_p(x4), _ld(x4), _p(y4), _ld(y4), B * H * W, Cc, int(x4.dtype == torch.float32),
                                         int(y4.dtype == torch.float32), code, _cmax_ptr(cmax, Cc), _stream()), "pf_copy_channels_ex")
            return
        check(_L.pf_copy_channels(_p(x4), _ld(x4), _p(y4), _ld(y4), B * H * W, Cc, int(x4.dtype == torch.float32),
                                  int(y4.dtype == torch.float32), code, _stream()), "pf_copy_channels")

    @staticmethod
    def pack_fusion_input(cdepth, fdepth, crops, y):
        B, h, w, c8 = y.shape
        assert c8 == 8 and y.is_contiguous() and cdepth.is_contiguous() and fdepth.is_contiguous() and crops.is_contiguous()
        check(_L.pf_pack_fusion_input(_p(cdepth), _p(fdepth), _p(crops), _p(y), B, h, w, _dt(y), _stream()), "pf_pack_fusion_input")

    @staticmethod
    def copy_plane(src, dst):
        """dst[...] = src[:, 0] for float32 depth planes (device-to-device, async on the current stream)"""
        dst.copy_(src[:, 0], non_blocking=True)

    @staticmethod
    def nhwc_to_nchw(x, Cc=None):
        B, H, W, Ct = x.shape
        Cc = Cc or Ct
        y = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
        code = 1 if x.dtype == torch.bfloat16 else 0
        check(_L.pf_nhwc_to_nchw_f32(_p(x), _ld(x), _p(y), B, H, W, Cc, int(x.dtype == torch.float32), code, _stream()), "pf_nhwc_to_nchw_f32")
        return y

    # ---------------- metric-bins head ----------------
    @staticmethod
    def attractor(A, n_attr, b_prev, out, a_stride=1, a_eps=0.0, attractor_type="inv", kind="mean"):
        """A [B,h,w,>=n_attr*a_stride] f32 ; b_prev [B,hp,wp,n_bins] f32 ; out [B,h,w,n_bins] f32 (include/pf_hip.h: pf_attractor)"""
        B, h, w, nb = out.shape
        _, hp, wp, _ = b_prev.shape
        assert A.dtype == b_prev.dtype == out.dtype == torch.float32 and b_prev.is_contiguous() and out.is_contiguous()
        assert A.shape[-1] >= (n_attr - 1) * a_stride + 1 and kind in ("mean", "sum")
        check(_L.pf_attractor(_p(A), _ld(A), n_attr, int(a_stride), float(a_eps), int(attractor_type == "exp"), int(kind == "sum"),
                              _p(b_prev), hp, wp, _p(out), B, h, w, nb, _stream()), "pf_attractor")

    @staticmethod
    def seed_bin_centers(x, out, min_depth, max_depth, bounded, normalize):
        """x [B,h,w,>=n_bins] f32 (relu / softplus MLP output) -> out [B,h,w,n_bins] f32 (include/pf_hip.h: pf_seed_bin_centers)"""
        assert x.dtype == out.dtype == torch.float32 and out.is_contiguous() and x.shape[:3] == out.shape[:3]
        check(_L.pf_seed_bin_centers(_p(x), _ld(x), _p(out), out.numel() // out.shape[-1], out.shape[-1], float(min_depth), float(max_depth),
                                     int(bool(bounded)), int(bool(normalize)), _stream()), "pf_seed_bin_centers")
        return out

    @staticmethod
    def bounded_bin_centers(b, out, min_depth, max_depth):
        """attractor.py:132-135: out = clip(sort((max - min) * b + min)) along the bins; b, out [B,h,w,n_bins] f32 contiguous"""
        assert b.dtype == out.dtype == torch.float32 and b.is_contiguous() and out.is_contiguous() and b.shape == out.shape
        check(_L.pf_bounded_bin_centers(_p(b), _p(out), out.numel() // out.shape[-1], out.shape[-1], float(min_depth), float(max_depth),
                                        _stream()), "pf_bounded_bin_centers")
        return out

    @staticmethod
    def logbinom_depth(pt, centers, depth, min_temp, max_temp):
        """pt [B,h,w,>=4] f32 (softplus applied); centers [B,hc,wc,n_bins] f32; depth [B,h,w] f32"""
        B, h, w = depth.shape
        _, hc, wc, nb = centers.shape
        assert pt.dtype == centers.dtype == depth.dtype == torch.float32 and centers.is_contiguous() and depth.is_contiguous()
        check(_L.pf_logbinom_depth(_p(pt), _ld(pt), _p(centers), hc, wc, _p(depth), B, h, w, nb, float(min_temp), float(max_temp), _stream()),
              "pf_logbinom_depth")

    @staticmethod
    def bins_tail(clb, emb, tw, centers, depth, min_temp, max_temp):
        """clb [B,H,W,ctot] f32 (channels [0,32) = last, [160,168) = rel when tw.nq == 11; the embedding slice is NOT read); emb [B,he,we,128]
        f32; tw packing.BinsTail; centers [B,hc,wc,64] f32; depth [B,H,W] f32"""
        B, H, W, _ = clb.shape
        _, he, we, ce = emb.shape
        _, hc, wc, nb = centers.shape
        assert clb.dtype == emb.dtype == centers.dtype == depth.dtype == torch.float32 and ce == 128 and nb == 64
        assert emb.is_contiguous() and centers.is_contiguous() and depth.is_contiguous() and clb.stride(3) == 1
        check(_L.pf_bins_tail(_p(clb), _ld(clb), tw.rel_off, _p(emb), he, we, _p(tw.w0f), _p(tw.b0), _p(tw.w2), _p(tw.b2), _p(centers), hc, wc,
                              _p(depth), B, H, W, tw.nq, float(min_temp), float(max_temp), _stream()), "pf_bins_tail")

    # ---------------- backward of the metric-bins head (csrc/head_bwd.hip; float32 only, fixed summation orders) ----------------
    @staticmethod
    def conv1x1_wgrad(dy, x, dw, db=None, rows_per_block=0):
        """dy [..., >=N] and x [..., >=K] float32 NHWC views over the same pixels (channel slices fine) -> dw [N, K] = sum_p dy x, db [N] = sum_p dy
        (include/pf_hip.h: pf_conv1x1_wgrad).  rows_per_block: pixels per partial tile, 0 = the library's default."""
        N, K = dw.shape
        dy4, x4 = _as4(dy), _as4(x)
        P = dy4.numel() // dy4.shape[-1]
        assert dy.dtype == x.dtype == dw.dtype == torch.float32 and dw.is_contiguous() and dy4.shape[:3] == x4.shape[:3]
        assert dy4.shape[-1] >= N and x4.shape[-1] >= K and (db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == N))
        need = C.c_long(0)
        check(_L.pf_conv1x1_wgrad_workspace_bytes(P, N, K, int(rows_per_block), C.byref(need)), "pf_conv1x1_wgrad_workspace_bytes")
        ws = torch.empty(need.value // 4, dtype=torch.float32, device=dw.device)
        check(_L.pf_conv1x1_wgrad(_p(dy4), _ld(dy4), _p(x4), _ld(x4), P, N, K, _p(dw), _p(db), _p(ws), need.value, int(rows_per_block), _stream()),
              "pf_conv1x1_wgrad")
        return dw, db

    @staticmethod
    def resize_bwd(dy, dx, accumulate=False):
        """adjoint of the align_corners=True bilinear resize: dy [B,OH,OW,C] -> dx [B,H,W,C] (+= with accumulate); float32, channel slices fine"""
        B, OH, OW, Cc = dy.shape
        Bx, H, W, Cx = dx.shape
        assert dy.dtype == dx.dtype == torch.float32 and B == Bx and Cc == Cx
        check(_L.pf_resize_bilinear_bwd(_p(dy), _ld(dy), B, OH, OW, Cc, _p(dx), _ld(dx), H, W, int(bool(accumulate)), _stream()),
              "pf_resize_bilinear_bwd")
        return dx

    @staticmethod
    def attractor_bwd(A, n_attr, b_prev, d_b_new, dA, d_b_c, attractor_type="inv", kind="mean"):
        """A [B,h,w,>=n_attr], b_prev [B,hp,wp,n_bins], d_b_new [B,h,w,n_bins] -> dA [B,h,w,>=n_attr], d_b_c [B,h,w,n_bins] (pf_attractor_bwd)"""
        B, h, w, nb = d_b_new.shape
        _, hp, wp, _ = b_prev.shape
        assert A.dtype == b_prev.dtype == d_b_new.dtype == dA.dtype == d_b_c.dtype == torch.float32 and kind in ("mean", "sum")
        assert b_prev.is_contiguous() and d_b_new.is_contiguous() and d_b_c.is_contiguous() and d_b_c.shape == d_b_new.shape
        assert A.shape[:3] == dA.shape[:3] == (B, h, w) and A.shape[-1] >= n_attr and dA.shape[-1] >= n_attr and b_prev.shape[-1] == nb
        check(_L.pf_attractor_bwd(_p(A), _ld(A), int(n_attr), int(attractor_type == "exp"), int(kind == "sum"), _p(b_prev), hp, wp, _p(d_b_new),
                                  _p(dA), _ld(dA), _p(d_b_c), B, h, w, nb, _stream()), "pf_attractor_bwd")
        return dA, d_b_c

    @staticmethod
    def logbinom_depth_bwd(pt, centers, d_depth, d_pt, d_centers_up, min_temp, max_temp):
        """pt [B,h,w,>=4] (softplus applied), centers [B,hc,wc,n_bins], d_depth [B,h,w] -> d_pt [B,h,w,>=4], d_centers_up [B,h,w,n_bins]"""
        B, h, w = d_depth.shape
        _, hc, wc, nb = centers.shape
        assert pt.dtype == centers.dtype == d_depth.dtype == d_pt.dtype == d_centers_up.dtype == torch.float32
        assert centers.is_contiguous() and d_depth.is_contiguous() and d_centers_up.is_contiguous() and tuple(d_centers_up.shape) == (B, h, w, nb)
        assert pt.shape[:3] == d_pt.shape[:3] == (B, h, w)
        check(_L.pf_logbinom_depth_bwd(_p(pt), _ld(pt), _p(centers), hc, wc, _p(d_depth), _p(d_pt), _ld(d_pt), _p(d_centers_up), B, h, w, nb,
                                       float(min_temp), float(max_temp), _p(_logbinom_logc(nb, pt.device)), _stream()), "pf_logbinom_depth_bwd")
        return d_pt, d_centers_up

    @staticmethod
    def act_bwd(dy, ref, act):
        """in place dy *= act'; ref = the layer's output for 'relu' / 'softplus', its pre-activation for 'gelu'; NHWC float32 views over the same pixels"""
        dy4, r4 = _as4(dy), _as4(ref)
        Cc = dy4.shape[-1]
        assert dy.dtype == ref.dtype == torch.float32 and dy4.shape[:3] == r4.shape[:3] and r4.shape[-1] >= Cc and act in ("relu", "gelu", "softplus")
        check(_L.pf_act_bwd(_p(dy4), _ld(dy4), _p(r4), _ld(r4), dy4.numel() // Cc, Cc, ACT[act], _stream()), "pf_act_bwd")
        return dy

    @staticmethod
    def silog_loss_saved(pred, target, min_depth, max_depth, beta=0.15):
        """silog_loss that also returns the three float64 sums (count, sum g, sum g^2) its backward needs -> (loss, sums)"""
        assert pred.dtype == target.dtype == torch.float32 and pred.shape == target.shape and pred.is_contiguous() and target.is_contiguous()
        ws = torch.empty(3, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        check(_L.pf_silog_loss(_p(pred), _p(target), pred.numel(), float(min_depth), float(max_depth), float(beta), _p(ws), _p(loss),
                               _stream()), "pf_silog_loss")
        return loss, ws

    @staticmethod
    def silog_loss_bwd(pred, target, sums, d_pred, min_depth, max_depth, beta=0.15, d_loss=1.0):
        """d_pred = d_loss * dL/dpred of silog_loss, from the sums silog_loss_saved returned; pred, target, d_pred float32 of equal shape"""
        assert pred.dtype == target.dtype == d_pred.dtype == torch.float32 and pred.shape == target.shape == d_pred.shape
        assert pred.is_contiguous() and target.is_contiguous() and d_pred.is_contiguous() and sums.dtype == torch.float64 and sums.numel() == 3
        check(_L.pf_silog_loss_bwd(_p(pred), _p(target), pred.numel(), float(min_depth), float(max_depth), float(beta), _p(sums), float(d_loss),
                                   _p(d_pred), _stream()), "pf_silog_loss_bwd")
        return d_pred

    # ---------------- stitching ----------------
    @staticmethod
    def stitch_init(pred, count, depth, mask, yx):
        MH, MW = pred.shape
        P, ph, pw = depth.shape
        assert depth.is_contiguous() and mask.is_contiguous() and yx.dtype == torch.int32
        check(_L.pf_stitch_init(_p(pred), _p(count), MH, MW, _p(depth), _p(mask), _p(yx), P, ph, pw, _stream()), "pf_stitch_init")

    @staticmethod
    def stitch_finish_init(avg, pred, count):
        check(_L.pf_stitch_finish_init(_p(avg), _p(pred), _p(count), avg.numel(), _stream()), "pf_stitch_finish_init")

    @staticmethod
    def stitch_update(avg, count, depth, mask, y0, x0):
        MH, MW = avg.shape
        dh, dw = depth.shape
        ph, pw = mask.shape
        assert depth.is_contiguous() and mask.is_contiguous()
        check(_L.pf_stitch_update(_p(avg), _p(count), MH, MW, _p(depth), dh, dw, _p(mask), int(y0), int(x0), ph, pw, _stream()), "pf_stitch_update")

    @staticmethod
    def resize_nearest_f32(x, y):
        check(_L.pf_resize_nearest_f32(_p(x), x.shape[0], x.shape[1], _p(y), y.shape[0], y.shape[1], _stream()), "pf_resize_nearest_f32")

    @staticmethod
    def resize_bilinear_f32(x, y):
        check(_L.pf_resize_bilinear_f32(_p(x), x.shape[0], x.shape[1], _p(y), y.shape[0], y.shape[1], _stream()), "pf_resize_bilinear_f32")

    # ---------------- input / output side (io.hip) ----------------
    @staticmethod
    def u8_bicubic_to_f32(img_u8, out, reverse_channels=False):
        """img_u8 [H,W,3] uint8 -> out [3,OH,OW] float32 (value/255, bicubic align_corners=True evaluated in double)."""
        assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous()
        assert out.dtype == torch.float32 and out.dim() == 3 and out.shape[0] == 3 and out.is_contiguous()
        check(_L.pf_u8_bicubic_to_f32(_p(img_u8), img_u8.shape[0], img_u8.shape[1], int(bool(reverse_channels)), _p(out), out.shape[1],
                                      out.shape[2], _stream()), "pf_u8_bicubic_to_f32")
        return out

    @staticmethod
    def percentiles(x, q0, q1, invalid_val=None, out=None, invalid_mask=None):
        """Exact np.percentile(x[x != invalid_val], [q0, q1]) (linear) of a float32 tensor -> device float32 [2];
        invalid_mask (uint8, same numel, non-zero = excluded) replaces the value test when given (color.py:121-122)."""
        assert x.dtype == torch.float32 and x.is_contiguous()
        if invalid_mask is not None:
            assert invalid_mask.dtype == torch.uint8 and invalid_mask.numel() == x.numel() and invalid_mask.is_contiguous()
        ws = torch.empty(_L.pf_percentile_workspace_bytes(), dtype=torch.uint8, device=x.device)
        out = torch.empty(2, dtype=torch.float32, device=x.device) if out is None else out
        check(_L.pf_percentiles_f32(_p(x), x.numel(), float(invalid_val if invalid_val is not None else 0.0), int(invalid_val is not None),
                                    _p(invalid_mask), float(q0), float(q1), _p(out), _p(ws), _stream()), "pf_percentiles_f32")
        return out

    @staticmethod
    def colorize(depth, vmin_vmax, lut_rgba, N, invalid_val, background_rgba, out, invalid_mask=None):
        assert depth.dtype == torch.float32 and depth.is_contiguous() and vmin_vmax.dtype == torch.float32 and vmin_vmax.numel() == 2
        assert lut_rgba.dtype == torch.uint8 and lut_rgba.shape == (N + 3, 4) and lut_rgba.is_contiguous()
        assert out.dtype == torch.uint8 and out.numel() == depth.numel() * 4 and out.is_contiguous()
        if invalid_mask is not None:
            assert invalid_mask.dtype == torch.uint8 and invalid_mask.numel() == depth.numel() and invalid_mask.is_contiguous()
        r, g, b, a = (int(v) & 255 for v in background_rgba)
        check(_L.pf_colorize_f32(_p(depth), depth.numel(), _p(vmin_vmax), _p(lut_rgba), int(N), float(invalid_val if invalid_val is not None else 0.0),
                                 int(invalid_val is not None), _p(invalid_mask), r | (g << 8) | (b << 16) | (a << 24), _p(out), _stream()),
              "pf_colorize_f32")
        return out

    @staticmethod
    def depth_to_u16(depth, out, scale=256.0):
        assert depth.dtype == torch.float32 and depth.is_contiguous() and out.dtype == torch.uint16 and out.numel() == depth.numel()
        check(_L.pf_depth_to_u16(_p(depth), depth.numel(), float(scale), _p(out), _stream()), "pf_depth_to_u16")
        return out

    @staticmethod
    def silog_loss(pred, target, min_depth, max_depth, beta=0.15):
        """SILogLoss forward (losses.py:15-62): pred, target float32 of equal shape -> device float32 scalar tensor"""
        assert pred.dtype == target.dtype == torch.float32 and pred.shape == target.shape and pred.is_contiguous() and target.is_contiguous()
        ws = torch.empty(3, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        check(_L.pf_silog_loss(_p(pred), _p(target), pred.numel(), float(min_depth), float(max_depth), float(beta), _p(ws), _p(loss),
                               _stream()), "pf_silog_loss")
        return loss

    @staticmethod
    def depth_metrics(gt, pred, edges, min_depth, max_depth, crop, out13, additional_mask=None):
        """gt [H,W], pred [h,w] float32, edges [H,W] float32 or None, crop = (y0, y1, x0, x1), additional_mask [H,W] uint8 or None
        (zero = excluded) -> out13 (device float64 [13])."""
        assert gt.dtype == torch.float32 and pred.dtype == torch.float32 and gt.dim() == 2 and pred.dim() == 2
        assert gt.is_contiguous() and pred.is_contiguous() and out13.dtype == torch.float64 and out13.numel() == 13
        if edges is not None:
            assert edges.dtype == torch.float32 and edges.shape == gt.shape and edges.is_contiguous()
        if additional_mask is not None:
            assert additional_mask.dtype == torch.uint8 and additional_mask.shape == gt.shape and additional_mask.is_contiguous()
        y0, y1, x0, x1 = (int(v) for v in crop)
        check(_L.pf_depth_metrics(_p(gt), gt.shape[0], gt.shape[1], _p(pred), pred.shape[0], pred.shape[1], _p(edges), _p(additional_mask),
                                  float(min_depth), float(max_depth), y0, y1, x0, x1, _p(out13), _stream()), "pf_depth_metrics")
        return out13

    # ---------------- evaluation side (evalops.hip) ----------------
    MAX_DILATION = 32
    COLOR_RGBA, COLOR_BGR = 0, 1

    @staticmethod
    def depth_boundaries(disp, th, dilation, out):
        """get_boundaries (image_ops.py:25-36): disp [H,W] float32 -> out [H,W] float32 of 0 / 1 (the `edges` plane of depth_metrics);
        dilation = side of the cv2.dilate box, 0 .. 32."""
        assert disp.dtype == torch.float32 and disp.dim() == 2 and disp.is_contiguous()
        assert out.dtype == torch.float32 and out.shape == disp.shape and out.is_contiguous() and out.data_ptr() != disp.data_ptr()
        dilation = int(dilation)
        if not 0 <= dilation <= HipOps.MAX_DILATION:
            raise ValueError(f"dilation {dilation} outside 0 .. {HipOps.MAX_DILATION}")
        check(_L.pf_depth_boundaries(_p(disp), 1, disp.shape[0], disp.shape[1], float(th), dilation, _p(out), _stream()), "pf_depth_boundaries")
        return out

    @staticmethod
    def colorize_ex(depth, vmin_vmax, lut_rgba, N, invalid_val, background_rgba, out, invalid_mask=None, layout=0):
        """colorize with an output layout: COLOR_RGBA -> out [n,4] (the bytes of colorize), COLOR_BGR -> out [n,3] = B, G, R"""
        assert layout in (HipOps.COLOR_RGBA, HipOps.COLOR_BGR)
        assert depth.dtype == torch.float32 and depth.is_contiguous() and vmin_vmax.dtype == torch.float32 and vmin_vmax.numel() == 2
        assert lut_rgba.dtype == torch.uint8 and lut_rgba.shape == (N + 3, 4) and lut_rgba.is_contiguous()
        assert out.dtype == torch.uint8 and out.numel() == depth.numel() * (4 if layout == HipOps.COLOR_RGBA else 3) and out.is_contiguous()
        if invalid_mask is not None:
            assert invalid_mask.dtype == torch.uint8 and invalid_mask.numel() == depth.numel() and invalid_mask.is_contiguous()
        r, g, b, a = (int(v) & 255 for v in background_rgba)
        check(_L.pf_colorize_f32_ex(_p(depth), depth.numel(), _p(vmin_vmax), _p(lut_rgba), int(N),
                                    float(invalid_val if invalid_val is not None else 0.0), int(invalid_val is not None), _p(invalid_mask),
                                    r | (g << 8) | (b << 16) | (a << 24), int(layout), _p(out), _stream()), "pf_colorize_f32_ex")
        return out

    # ---------------- PNG encoding of the saved images (png.hip) ----------------
    PNG_BAND_ROWS, PNG_TABLE_WORDS = 8, 324

    @staticmethod
    def png_format(image, bgr=False):
        """uint8 [H,W] / [H,W,3] / [H,W,4] or uint16 [H,W] -> (H, W, channels, bits, bgr)"""
        if image.dtype == torch.uint8 and image.dim() in (2, 3):
            ch, bits = (1 if image.dim() == 2 else int(image.shape[2])), 8
        elif image.dtype == torch.uint16 and image.dim() == 2:
            ch, bits = 1, 16
        else:
            raise ValueError(f"png: expected uint8 [H,W], [H,W,3], [H,W,4] or uint16 [H,W], got {image.dtype} {tuple(image.shape)}")
        if ch not in (1, 3, 4) or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(f"png: unsupported shape {tuple(image.shape)}")
        if bgr and ch < 3:
            raise ValueError("png: bgr needs three or four channels")
        assert image.is_contiguous()
        return int(image.shape[0]), int(image.shape[1]), ch, bits, int(bool(bgr))

    @staticmethod
    def png_workspace(image, bgr=False):
        """-> (workspace bytes, output bytes, number of bands) of the PNG encoder for this image"""
        H, W, ch, bits, _ = HipOps.png_format(image, bgr)
        ws, ob, nb = C.c_long(), C.c_long(), C.c_int()
        check(_L.pf_png_workspace_bytes(H, W, ch, bits, C.byref(ws), C.byref(ob), C.byref(nb)), "pf_png_workspace_bytes")
        return ws.value, ob.value, nb.value

    @staticmethod
    def png_filter_histogram(image, workspace, hist, bgr=False):
        """pass A: the row filters go into `workspace` (uint8, png_workspace bytes), the 257 counts into `hist` (int32 [257], device)"""
        H, W, ch, bits, bgr = HipOps.png_format(image, bgr)
        assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= HipOps.png_workspace(image)[0]
        assert hist.dtype == torch.int32 and hist.numel() == 257 and hist.is_contiguous()
        check(_L.pf_png_filter_histogram(_p(image), H, W, ch, bits, bgr, _p(workspace), _p(hist), _stream()), "pf_png_filter_histogram")
        return hist

    @staticmethod
    def png_build_table(hist):
        """host step: 257 counts (sequence / numpy / host tensor) -> numpy uint32 [PNG_TABLE_WORDS] (codes, header bits, header)"""
        import numpy as np
        h = np.ascontiguousarray(np.asarray(hist, dtype=np.int64).reshape(-1).astype(np.uint32))
        assert h.size == 257
        table = np.zeros(HipOps.PNG_TABLE_WORDS, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        check(_L.pf_png_build_table(h.ctypes.data_as(u32p), table.ctypes.data_as(u32p)), "pf_png_build_table")
        return table

    @staticmethod
    def png_encode(image, table, workspace, out, meta, bgr=False):
        """pass B + C: table int32 [PNG_TABLE_WORDS] on the device; out uint8 (png_workspace output bytes) receives the deflate blocks of
        all bands back to back, meta int32 [2 + 3 * bands] the total size and each band's {bytes, Adler S1, S2}"""
        H, W, ch, bits, bgr = HipOps.png_format(image, bgr)
        assert table.dtype == torch.int32 and table.numel() == HipOps.PNG_TABLE_WORDS and table.is_contiguous()
        ws_bytes, out_bytes, nbands = HipOps.png_workspace(image)
        assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= ws_bytes
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= out_bytes
        assert meta.dtype == torch.int32 and meta.is_contiguous() and meta.numel() >= 2 + 3 * nbands
        check(_L.pf_png_encode(_p(image), H, W, ch, bits, bgr, _p(table), _p(workspace), _p(out), _p(meta), _stream()), "pf_png_encode")
        return out, meta

    # ---------------- the same with run matches at distance 1 (png_rle.hip) ----------------
    PNG_RLE_TABLE_WORDS, PNG_RLE_HIST_WORDS = 388, 546

    @staticmethod
    def png_rle_workspace(image, bgr=False):
        """png_workspace sized for the larger slot of the two codings: serves png_encode as well as png_rle_encode"""
        H, W, ch, bits, _ = HipOps.png_format(image, bgr)
        ws, ob, nb = C.c_long(), C.c_long(), C.c_int()
        check(_L.pf_png_rle_workspace_bytes(H, W, ch, bits, C.byref(ws), C.byref(ob), C.byref(nb)), "pf_png_rle_workspace_bytes")
        return ws.value, ob.value, nb.value

    @staticmethod
    def png_rle_filter_histogram(image, workspace, hist, bgr=False):
        """pass A': png_filter_histogram's filters; hist (int32 [PNG_RLE_HIST_WORDS], device) = 257 literal counts, 286 token counts
        from [257], the matches' extra bits as 64 bits from [544]"""
        H, W, ch, bits, bgr = HipOps.png_format(image, bgr)
        assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= HipOps.png_rle_workspace(image)[0]
        assert hist.dtype == torch.int32 and hist.numel() == HipOps.PNG_RLE_HIST_WORDS and hist.is_contiguous()
        check(_L.pf_png_rle_filter_histogram(_p(image), H, W, ch, bits, bgr, _p(workspace), _p(hist), _stream()), "pf_png_rle_filter_histogram")
        return hist

    @staticmethod
    def png_rle_build_table(hist):
        """host step: 286 token counts -> numpy uint32 [PNG_RLE_TABLE_WORDS] (codes <= 14 bits, length symbols, header)"""
        import numpy as np
        h = np.ascontiguousarray(np.asarray(hist, dtype=np.int64).reshape(-1).astype(np.uint32))
        assert h.size == 286
        table = np.zeros(HipOps.PNG_RLE_TABLE_WORDS, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        check(_L.pf_png_rle_build_table(h.ctypes.data_as(u32p), table.ctypes.data_as(u32p)), "pf_png_rle_build_table")
        return table

    @staticmethod
    def png_rle_encode(image, table, workspace, out, meta, bgr=False):
        """pass B' + C: png_encode with the table of png_rle_build_table (int32 [PNG_RLE_TABLE_WORDS], device)"""
        H, W, ch, bits, bgr = HipOps.png_format(image, bgr)
        assert table.dtype == torch.int32 and table.numel() == HipOps.PNG_RLE_TABLE_WORDS and table.is_contiguous()
        ws_bytes, out_bytes, nbands = HipOps.png_rle_workspace(image)
        assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= ws_bytes
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= out_bytes
        assert meta.dtype == torch.int32 and meta.is_contiguous() and meta.numel() >= 2 + 3 * nbands
        check(_L.pf_png_rle_encode(_p(image), H, W, ch, bits, bgr, _p(table), _p(workspace), _p(out), _p(meta), _stream()), "pf_png_rle_encode")
        return out, meta

    # ---------------- JPEG decoding of the input image (jpeg.hip); the host steps live in preprocess.JpegHost ----------------
    JPEG_TABLE_WORDS, JPEG_E_STREAM, JPEG_NOT_CONVERGED = 2152, 48, 64     # PF_JPEG_TABLE_WORDS, PF_JPEG_E_STREAM, PF_JPEG_NOT_CONVERGED

    @staticmethod
    def jpeg_workspace(header, nlanes):
        """-> (entropy workspace bytes, reconstruction workspace bytes)"""
        a, b = C.c_long(), C.c_long()
        check(_L.pf_jpeg_workspace_bytes(C.byref(header), int(nlanes), C.byref(a), C.byref(b)), "pf_jpeg_workspace_bytes")
        return a.value, b.value

    @staticmethod
    def jpeg_decode_entropy(header, scan, lanes, segx, longest, tables, max_sync_rounds, workspace, coef):
        """scan uint8, lanes int32 [nlanes,3], segx int32 [nsegments,4], tables int32, workspace uint8, coef int16 [nblocks,64], all on the
        device -> (status, sync rounds); status 0, PF_JPEG_E_STREAM or PF_JPEG_NOT_CONVERGED (anything else raises)"""
        nlanes = int(lanes.shape[0])
        assert scan.dtype == torch.uint8 and lanes.dtype == torch.int32 and segx.dtype == torch.int32 and tables.dtype == torch.int32
        assert all(t.is_contiguous() for t in (scan, lanes, segx, tables, workspace, coef))
        assert coef.dtype == torch.int16 and coef.numel() == header.nblocks * 64 and segx.shape[0] == header.nsegments
        assert tables.numel() == HipOps.JPEG_TABLE_WORDS
        assert workspace.dtype == torch.uint8 and workspace.numel() >= HipOps.jpeg_workspace(header, nlanes)[0]
        rounds = C.c_int()
        rc = _L.pf_jpeg_decode_entropy(C.byref(header), _p(scan), scan.numel(), _p(lanes), _p(segx), nlanes, int(longest), _p(tables),
                                       int(max_sync_rounds), _p(workspace), _p(coef), C.byref(rounds), _stream())
        if rc not in (0, HipOps.JPEG_E_STREAM, HipOps.JPEG_NOT_CONVERGED):
            check(rc, "pf_jpeg_decode_entropy")
        return rc, rounds.value

    @staticmethod
    def jpeg_reconstruct(header, coef, orientation, workspace, rgb):
        """coef int16 [nblocks,64] -> rgb uint8 [H',W',3] (both on the device)"""
        H, W = (header.width, header.height) if orientation >= 5 else (header.height, header.width)
        assert coef.dtype == torch.int16 and coef.is_contiguous() and coef.numel() == header.nblocks * 64
        assert rgb.dtype == torch.uint8 and rgb.is_contiguous() and tuple(rgb.shape) == (H, W, 3)
        assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= HipOps.jpeg_workspace(header, 0)[1]
        check(_L.pf_jpeg_reconstruct(C.byref(header), _p(coef), int(orientation), _p(workspace), _p(rgb), _stream()), "pf_jpeg_reconstruct")
        return rgb

    # ---------------- progressive JPEG (jpeg_prog.hip); the host steps live in preprocess.JpegProgHost ----------------
    @staticmethod
    def jpeg_prog_workspace(nlanes, scan_blocks):
        n = C.c_long()
        check(_L.pf_jpeg_prog_workspace_bytes(int(nlanes), int(scan_blocks), C.byref(n)), "pf_jpeg_prog_workspace_bytes")
        return n.value

    @staticmethod
    def jpeg_prog_decode_scan(header, scan, data, lanes, segx, longest, tables, block_map, max_sync_rounds, workspace, coef):
        """a DC-first or AC-first scan: data uint8, lanes int32 [nlanes,3], segx int32 [nsegments,4], tables int32, block_map int32 [scan
        blocks] or None (interleaved scan), workspace uint8, coef int16 [nblocks,64] (not zeroed here), all on the device -> (status,
        sync rounds); status 0, PF_JPEG_E_STREAM or PF_JPEG_NOT_CONVERGED (anything else raises)"""
        nlanes = int(lanes.shape[0])
        assert data.dtype == torch.uint8 and lanes.dtype == torch.int32 and segx.dtype == torch.int32 and tables.dtype == torch.int32
        assert all(t.is_contiguous() for t in (data, lanes, segx, tables, workspace, coef))
        assert coef.dtype == torch.int16 and coef.numel() == header.nblocks * 64 and segx.shape[0] == scan.nsegments
        assert tables.numel() == HipOps.JPEG_TABLE_WORDS
        assert block_map is None or (block_map.dtype == torch.int32 and block_map.is_contiguous() and block_map.numel() == scan.nblocks)
        assert workspace.dtype == torch.uint8 and workspace.numel() >= HipOps.jpeg_prog_workspace(nlanes, scan.nblocks)
        rounds = C.c_int()
        rc = _L.pf_jpeg_prog_decode_scan(C.byref(header), C.byref(scan), _p(data), data.numel(), _p(lanes), _p(segx), nlanes, int(longest),
                                         _p(tables), None if block_map is None else _p(block_map), int(max_sync_rounds), _p(workspace), _p(coef),
                                         C.byref(rounds), _stream())
        if rc not in (0, HipOps.JPEG_E_STREAM, HipOps.JPEG_NOT_CONVERGED):
            check(rc, "pf_jpeg_prog_decode_scan")
        return rc, rounds.value

    @staticmethod
    def jpeg_prog_dc_refine(header, scan, data, segs, block_map, coef):
        """a DC-refinement scan: data uint8, segs int32 [nsegments,2] on the device"""
        assert data.dtype == torch.uint8 and data.is_contiguous() and segs.dtype == torch.int32 and segs.is_contiguous()
        assert segs.numel() == 2 * scan.nsegments and coef.dtype == torch.int16 and coef.is_contiguous() and coef.numel() == header.nblocks * 64
        assert block_map is None or (block_map.dtype == torch.int32 and block_map.is_contiguous() and block_map.numel() == scan.nblocks)
        check(_L.pf_jpeg_prog_dc_refine(C.byref(header), C.byref(scan), _p(data), data.numel(), _p(segs), None if block_map is None else _p(block_map),
                                        _p(coef), _stream()), "pf_jpeg_prog_dc_refine")

    @staticmethod
    def jpeg_prog_nonzero_mask(header, scan, coef, block_map, masks):
        """coef -> masks int64 [scan blocks] (device): bit i = coefficient i of the block is non-zero"""
        assert coef.dtype == torch.int16 and coef.is_contiguous() and coef.numel() == header.nblocks * 64
        assert masks.dtype == torch.int64 and masks.is_contiguous() and masks.numel() == scan.nblocks
        assert block_map.dtype == torch.int32 and block_map.is_contiguous() and block_map.numel() == scan.nblocks
        check(_L.pf_jpeg_prog_nonzero_mask(C.byref(header), C.byref(scan), _p(coef), _p(block_map), _p(masks), _stream()), "pf_jpeg_prog_nonzero_mask")
        return masks

    @staticmethod
    def jpeg_prog_apply_refinement(header, scan, records, block_map, coef):
        """records int64 [scan blocks,3] (device) of an AC-refinement scan -> coef"""
        assert coef.dtype == torch.int16 and coef.is_contiguous() and coef.numel() == header.nblocks * 64
        assert records.dtype == torch.int64 and records.is_contiguous() and records.numel() == 3 * scan.nblocks
        assert block_map.dtype == torch.int32 and block_map.is_contiguous() and block_map.numel() == scan.nblocks
        check(_L.pf_jpeg_prog_apply_refinement(C.byref(header), C.byref(scan), _p(records), _p(block_map), _p(coef), _stream()),
              "pf_jpeg_prog_apply_refinement")

    # ---------------- PNG decoding of the input image (png_decode.hip); parse and chain walk live in preprocess ----------------
    @staticmethod
    def pngd_find(words, nbits, cand, count):
        """words int32 (the deflate stream, zero padded by PF_PNGD_PAD_WORDS words) -> cand int32 [capacity] and count int32 [1] (keeps counting past
        the capacity), all on the device"""
        assert words.dtype == torch.int32 and cand.dtype == torch.int32 and count.dtype == torch.int32 and count.numel() == 1
        assert words.is_contiguous() and cand.is_contiguous() and 0 < nbits <= 32 * (words.numel() - 2)
        check(_L.pf_pngd_find(_p(words), words.numel(), int(nbits), _p(cand), cand.numel(), _p(count), _stream()), "pf_pngd_find")

    @staticmethod
    def pngd_scan(words, nbits, starts, n, max_block_bits, expected, records):
        """starts int32 [>= n] -> records int32 [n,4] = {start bit, end bit, output bytes, status | BFINAL << 8}"""
        assert words.dtype == torch.int32 and starts.dtype == torch.int32 and records.dtype == torch.int32
        assert words.is_contiguous() and starts.is_contiguous() and records.is_contiguous() and 0 < nbits <= 32 * (words.numel() - 2)
        assert 0 <= n <= starts.numel() and records.numel() >= 4 * n
        check(_L.pf_pngd_scan(_p(words), words.numel(), int(nbits), _p(starts), int(n), int(max_block_bits), int(expected), _p(records), _stream()), "pf_pngd_scan")
        return records

    @staticmethod
    def pngd_inflate(words, nbits, blocks, expected, lit, ref, status):
        """blocks int32 [nblocks,4] = {start, type, output offset, output bytes} -> lit uint8 [expected], ref int32 [expected]"""
        assert words.dtype == torch.int32 and blocks.dtype == torch.int32 and lit.dtype == torch.uint8 and ref.dtype == torch.int32
        assert all(t.is_contiguous() for t in (words, blocks, lit, ref)) and 0 < nbits <= 32 * (words.numel() - 2)
        assert blocks.dim() == 2 and blocks.shape[1] == 4 and lit.numel() == expected and ref.numel() == expected
        assert status.dtype == torch.int32 and status.numel() >= 1
        check(_L.pf_pngd_inflate(_p(words), words.numel(), int(nbits), _p(blocks), blocks.shape[0], int(expected), _p(lit), _p(ref), _p(status), _stream()),
              "pf_pngd_inflate")

    @staticmethod
    def pngd_scan_par(words, nbits, starts, n, max_block_bits, expected, subsequence_bits, records, max_rounds):
        """pngd_scan with the symbols of a block decoded in lanes of subsequence_bits bits (png_inflate_par.hip): the same records wherever
        pngd_scan's status is OK; max_rounds int32 [1] (zeroed by the caller) is raised to the largest number of rounds a window needed"""
        assert words.dtype == torch.int32 and starts.dtype == torch.int32 and records.dtype == torch.int32
        assert words.is_contiguous() and starts.is_contiguous() and records.is_contiguous() and 0 < nbits <= 32 * (words.numel() - 2)
        assert 0 <= n <= starts.numel() and records.numel() >= 4 * n and max_rounds.dtype == torch.int32 and max_rounds.numel() >= 1
        check(_L.pf_pngd_scan_par(_p(words), words.numel(), int(nbits), _p(starts), int(n), int(max_block_bits), int(expected), int(subsequence_bits),
                                  _p(records), _p(max_rounds), _stream()), "pf_pngd_scan_par")
        return records

    @staticmethod
    def pngd_inflate_par(words, nbits, blocks, expected, subsequence_bits, lit, ref, status, max_rounds):
        """pngd_inflate with one workgroup per block and one lane of subsequence_bits bits per thread; afterwards a reference points to a literal
        or into a strictly earlier lane's range"""
        assert words.dtype == torch.int32 and blocks.dtype == torch.int32 and lit.dtype == torch.uint8 and ref.dtype == torch.int32
        assert all(t.is_contiguous() for t in (words, blocks, lit, ref)) and 0 < nbits <= 32 * (words.numel() - 2)
        assert blocks.dim() == 2 and blocks.shape[1] == 4 and lit.numel() == expected and ref.numel() == expected
        assert status.dtype == torch.int32 and status.numel() >= 1 and max_rounds.dtype == torch.int32 and max_rounds.numel() >= 1
        check(_L.pf_pngd_inflate_par(_p(words), words.numel(), int(nbits), _p(blocks), blocks.shape[0], int(expected), int(subsequence_bits), _p(lit),
                                     _p(ref), _p(status), _p(max_rounds), _stream()), "pf_pngd_inflate_par")

    @staticmethod
    def pngd_resolve(lit, ref, rounds, out):
        """`rounds` pointer-jumping launches over ref (in place), then out[i] = lit[ref[i]]"""
        assert lit.dtype == torch.uint8 and ref.dtype == torch.int32 and out.dtype == torch.uint8
        assert lit.is_contiguous() and ref.is_contiguous() and out.is_contiguous() and lit.numel() == ref.numel() == out.numel()
        check(_L.pf_pngd_resolve(_p(lit), _p(ref), ref.numel(), int(rounds), _p(out), _stream()), "pf_pngd_resolve")
        return out

    @staticmethod
    def pngd_unfilter(header, inflated, recon, status):
        """inflated uint8 [height * (1 + rowbytes)] -> recon uint8 [height * rowbytes]"""
        assert inflated.dtype == torch.uint8 and inflated.is_contiguous() and inflated.numel() == header.inflated_bytes
        assert recon.is_contiguous() and recon.numel() * recon.element_size() == header.height * header.rowbytes
        assert status.dtype == torch.int32 and status.numel() >= 1
        check(_L.pf_pngd_unfilter(_p(inflated), C.byref(header), _p(recon), _p(status), _stream()), "pf_pngd_unfilter")
        return recon

    @staticmethod
    def pngd_expand(header, recon, palette, image, status):
        """recon -> image for sub-byte samples, a palette (uint8 [768] on the device, else None) and 16-bit samples"""
        assert recon.dtype == torch.uint8 and recon.is_contiguous() and recon.numel() == header.height * header.rowbytes
        out_ch = 3 if header.color_type == 3 else header.channels
        assert image.is_contiguous() and image.numel() == header.height * header.width * out_ch
        assert image.element_size() == (2 if header.depth == 16 else 1)
        assert palette is None or (palette.dtype == torch.uint8 and palette.numel() == 768 and palette.is_contiguous())
        check(_L.pf_pngd_expand(_p(recon), C.byref(header), None if palette is None else _p(palette), _p(image), _p(status), _stream()),
              "pf_pngd_expand")
        return image

    @staticmethod
    def pngd_adler(data, sums, result):
        """Adler-32 of data (uint8, device) -> result int32 [>= 1]; sums: int64 [2] of workspace"""
        assert data.dtype == torch.uint8 and data.is_contiguous() and sums.dtype == torch.int64 and sums.numel() >= 2 and result.dtype == torch.int32
        check(_L.pf_pngd_adler(_p(data), data.numel(), _p(sums), _p(result), _stream()), "pf_pngd_adler")

    @staticmethod
    def pngd_to_rgb8(image, rgb):
        """a decoded PNG (uint8 or uint16; [H,W] or [H,W,C]) -> rgb uint8 [H,W,3]: grey replicated, alpha dropped, the high byte of 16 bits"""
        H, W = image.shape[0], image.shape[1]
        ch = 1 if image.dim() == 2 else image.shape[2]
        assert image.is_contiguous() and image.element_size() in (1, 2) and rgb.dtype == torch.uint8 and rgb.is_contiguous()
        assert tuple(rgb.shape) == (H, W, 3)
        check(_L.pf_pngd_to_rgb8(_p(image), H, W, ch, 8 * image.element_size(), _p(rgb), _stream()), "pf_pngd_to_rgb8")
        return rgb

    # ---------------- ground-truth depth files (gtread.hip) ----------------
    GT_KINDS = {"f2": 0, "f4": 1, "f8": 2, "u1": 3, "u2": 4}                       # PF_GT_F16 .. PF_GT_U16
    GT_KIND_BYTES = {"f2": 2, "f4": 4, "f8": 8, "u1": 1, "u2": 2}
    GT_MODES = {"u4k": 0, "mid": 1, "eth3d": 2, "gta": 3, "cityscapes": 4, "raw": 5}   # PF_GT_U4K .. PF_GT_RAW
    GT_SWAP, GT_FLIP = 1, 2

    @staticmethod
    def gt_convert(src, kind, mode, H, W, a, b, depth, edge_src=None, swap=False, flip=False):
        """The payload of a ground-truth file (src: the bytes as uint8, or a decoded uint8 / uint16 image; H * W samples of `kind` =
        'f2' 'f4' 'f8' 'u1' 'u2') -> depth float32 [H,W] and, when given, the plane get_boundaries takes; the arithmetic per `mode` is
        the table of include/pf_hip.h.  a, b: the mode's constants, rounded to float32 on the way in."""
        if kind not in HipOps.GT_KINDS or mode not in HipOps.GT_MODES:
            raise ValueError(f"gt_convert: unknown kind {kind!r} or mode {mode!r}")
        H, W = int(H), int(W)
        assert src.is_contiguous() and src.numel() * src.element_size() == H * W * HipOps.GT_KIND_BYTES[kind], "payload size"
        for t in (depth, edge_src):
            assert t is None or (t.dtype == torch.float32 and tuple(t.shape) == (H, W) and t.is_contiguous())
        assert edge_src is None or edge_src.data_ptr() != depth.data_ptr()
        flags = (HipOps.GT_SWAP if swap else 0) | (HipOps.GT_FLIP if flip else 0)
        check(_L.pf_gt_convert(_p(src), HipOps.GT_KINDS[kind], flags, HipOps.GT_MODES[mode], H, W, float(a), float(b), _p(depth), _p(edge_src),
                               _stream()), "pf_gt_convert")
        return depth

    # ---------------- training-side augmentations (augment.hip) ----------------
    @staticmethod
    def aug_image_u8_to_f32(img_u8, matrix, flip, colour, out):
        """img_u8 uint8 [H,W,3] in the raw file's order (B, G, R) -> out float32 [3,H,W] (R, G, B): Pillow's bilinear rotation with
        Image.rotate's `matrix` (six Python floats), the flip, / 255 and, when colour = (gamma, brightness, (cr, cg, cb)) is not None,
        aug_color's arithmetic (include/pf_hip.h).  gamma and brightness are rounded to float32 on the way in, as numpy does."""
        H, W = img_u8.shape[0], img_u8.shape[1]
        assert img_u8.dtype == torch.uint8 and tuple(img_u8.shape) == (H, W, 3) and img_u8.is_contiguous()
        assert out.dtype == torch.float32 and tuple(out.shape) == (3, H, W) and out.is_contiguous()
        m = (C.c_double * 6)(*[float(v) for v in matrix])
        gamma, brightness, colours = colour if colour is not None else (1.0, 1.0, (1.0, 1.0, 1.0))
        col = (C.c_double * 3)(*[float(v) for v in colours])
        check(_L.pf_aug_image_u8_to_f32(_p(img_u8), H, W, m, int(bool(flip)), int(colour is not None), float(gamma), float(brightness), col,
                                        _p(out), _stream()), "pf_aug_image_u8_to_f32")
        return out

    @staticmethod
    def aug_planes_nearest(srcs, fixed, flip, outs):
        """one or two float32 [H,W] planes -> the same rotated by Pillow's nearest-neighbour fixed-point path (`fixed`: the six 16.16
        integers of include/pf_hip.h) and flipped; 0 outside the source"""
        assert len(srcs) == len(outs) and len(srcs) in (1, 2)
        H, W = srcs[0].shape
        for t in tuple(srcs) + tuple(outs):
            assert t.dtype == torch.float32 and tuple(t.shape) == (H, W) and t.is_contiguous()
        a = [int(v) for v in fixed]
        if len(a) != 6 or any(abs(v) >= 2 ** 31 for v in a):
            raise ValueError(f"aug_planes_nearest: six 16.16 integers inside int32 are expected, got {fixed!r}")
        check(_L.pf_aug_planes_nearest(_p(srcs[0]), _p(srcs[1]) if len(srcs) == 2 else None, H, W, (C.c_int * 6)(*a), int(bool(flip)),
                                       _p(outs[0]), _p(outs[1]) if len(outs) == 2 else None, _stream()), "pf_aug_planes_nearest")
        return outs


ops = HipOps()
