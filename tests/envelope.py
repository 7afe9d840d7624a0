"""The argument envelope of the inference engine's C entry points (include/pf_hip.h), as data -- not a test module.

One entry per `extern "C"` function defined in the sources of SOURCES:
  good     a small valid call: argument name -> value.  Pointer arguments are listed in `ptrs` (name -> bytes of the widest access the kernel makes
           through it; a name in `optional` may be null) and get their value from a provider -- made-up aligned addresses on the CPU.  The fields of
           a pf_conv_params argument are written "p.<field>".  HOST arrays (arguments the launcher itself reads) are given as ctypes objects.
  refused  named mutations of `good` that must return PF_ERR_ARG (queries: their "no" value, `no`).  rows() adds, for EVERY pointer, the null call
           and the call with the pointer moved off its boundary by half the access width -- so "every pointer" cannot be forgotten -- and the
           coverage test (tests/test_envelope_refusals_cpu.py) demands a mutation of every integer argument.
  corners  the accepted edge shapes tests/test_envelope_corners_gpu.py runs on the device (ids of its cases), or `no_corner`: why there is none.

Nothing here launches: tests/test_envelope_refusals_cpu.py sends the rows to the library on a machine WITHOUT a device only, where a call that slips
through the checks ends in PF_ERR_LAUNCH instead of running on made-up addresses."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("igemm", "winograd", "wino_fused", "wino_f16x2", "wino_f16x2_n256", "gemm_split3", "gemm_f16x2_t160", "conv1x1_split3", "attn_split3",
           "vit", "swin", "imageops", "beit", "beit_bf16")
PF_ERR_ARG = 1
NO_ARGUMENTS = {"pf_last_error": "takes no argument", "pf_version": "takes no argument", "pf_conv_last_variant": "takes no argument"}
# arguments any value of which is legal (flags read as booleans, free floats, the stream)
FREE = {"stream", "eps", "scale", "a_eps", "min_depth", "max_depth", "min_temp", "max_temp", "relu_in", "in_f32", "out_f32", "kmajor", "attractor_exp",
        "kind_sum", "bounded", "normalize", "cmax_out_relu", "maxima_given", "grid_cap", "p.relu_in", "p.out_f32"}
INT32, INT31 = 1 << 32, 1 << 31


def source_of():
    """entry point -> source file, from the extern "C" definitions of SOURCES"""
    out = {}
    for src in SOURCES:
        txt = open(os.path.join(ROOT, "patchfusion_amd", "csrc", src + ".hip")).read()
        txt = re.sub(r"#ifdef PF_ATTN_DBG\n// decomposition build only.*?#endif", "", txt, flags=re.S)
        for name in re.findall(r'^extern "C" [\w \*]+?\b(pf_\w+)\s*\(', txt, flags=re.M):
            out[name] = src + ".hip"
    return out


def prototypes():
    """entry point -> [(type, name)] for every in-scope function declared in include/pf_hip.h"""
    txt = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    scope = source_of()
    out = {}
    for m in re.finditer(r"\b(?:int|long|const char\*)\s+(pf_\w+)\s*\(([^)]*)\)\s*;", txt):
        name, args = m.group(1), m.group(2).strip()
        if name not in scope:
            continue
        plist = []
        for a in ([] if args in ("", "void") else args.split(",")):
            a = " ".join(a.split())
            am = re.match(r"(.*?)(\w+)$", a)
            plist.append((am.group(1).strip(), am.group(2)))
        out[name] = plist
    return out


CONV_INT_FIELDS = ("x_ld", "B", "H", "W", "Cin", "w_rows", "Kpad", "res_ld", "res2_ld", "y_ld", "OH", "OW", "Cout", "KH", "KW", "stride", "pad", "act",
                   "relu_in", "out_f32", "shuffle", "dtype", "korder", "batch", "x_bstride", "w_bstride", "y_bstride")
CONV_PTR_FIELDS = ("x", "w", "bias", "scale", "res", "res2", "y", "col_exp", "out_exp")

TABLE = {}


def entry(name, good, ptrs, refused, optional=(), corners=(), no_corner=None, no=PF_ERR_ARG, reads=None, query=False):
    """reads: the pf_conv_params fields the entry point looks at (None: all); a field outside it needs no mutation"""
    assert name not in TABLE, name
    TABLE[name] = dict(good=good, ptrs=ptrs, refused=refused, optional=set(optional), corners=tuple(corners), no_corner=no_corner, no=no, reads=reads,
                       query=query)


def fake_pointers():
    """made-up, generously aligned, non-null addresses, one 1 MiB slot per pointer"""
    n = [0]

    def ptr(name, align):
        n[0] += 1
        return 0x10000000 + n[0] * 0x100000
    return ptr


def rows(name):
    """-> [(row id, {argument: value | 'NULL' | ('OFF', bytes)})] for an entry: the table's mutations plus the null / misaligned row of every pointer"""
    e = TABLE[name]
    out = [(k, dict(v)) for k, v in e["refused"].items()]
    if e["query"]:
        return out
    for p, width in e["ptrs"].items():
        if width == "host":
            out.append((f"null:{p}", {p: "NULL"}))
            continue
        if p not in e["optional"]:
            out.append((f"null:{p}", {p: "NULL"}))
        if width >= 2:
            out.append((f"misaligned:{p}", {p: ("OFF", width // 2)}))
    return out


def build(name, lib_mod, ptr, mutation=None):
    """-> (the argument tuple for the ctypes function, objects to keep alive) of `good` with `mutation` applied"""
    e = TABLE[name]
    vals = dict(e["good"])
    for p, width in e["ptrs"].items():
        if width != "host" and p not in vals:
            vals[p] = None if p in e["optional"] else ptr(p, width)      # (an optional operand is absent from the good call)
    for k, v in (mutation or {}).items():
        if isinstance(v, str) and v == "NULL":
            vals[k] = None
        elif isinstance(v, tuple) and v[0] == "OFF":
            base = vals[k] if vals.get(k) is not None else ptr(k, 2 * v[1])
            vals[k] = (C.cast(base, C.c_void_p).value if not isinstance(base, int) else base) + v[1]
        else:
            vals[k] = v
    keep, args = [], []
    for ctype, an in prototypes()[name]:
        if "pf_conv_params" in ctype:
            if vals.get(an, 1) is None:
                args.append(None)
                continue
            st = lib_mod.ConvParams()
            for f in CONV_INT_FIELDS + CONV_PTR_FIELDS:
                v = vals.get(f"{an}.{f}")
                if v is not None:
                    setattr(st, f, v)
            keep.append(st)
            args.append(C.byref(st))
        elif an == "stream":
            args.append(None)
        else:
            v = vals[an]
            if isinstance(v, float):
                v = C.c_float(v)
            elif ctype in ("const int*", "const void* const*", "float*") and isinstance(v, int):
                v = C.cast(C.c_void_p(v), _pointer_type(ctype))
            elif v is not None and not isinstance(v, int):
                keep.append(v)
            args.append(v)
    return tuple(args), keep


def _pointer_type(ctype):
    return {"const int*": C.POINTER(C.c_int), "const void* const*": C.POINTER(C.c_void_p), "float*": C.POINTER(C.c_float)}[ctype]


def call(lib, lib_mod, name, ptr, mutation=None):
    args, keep = build(name, lib_mod, ptr, mutation)
    fn = getattr(lib, name)
    try:
        return fn(*args)
    except C.ArgumentError:
        # entry points bound with typed pointers (POINTER(c_int) ...) take the raw address through a cast
        sig = lib_mod.SIGNATURES.get(name)
        cast = [C.cast(C.c_void_p(a), t) if isinstance(a, int) and hasattr(t, "contents") else a for a, t in zip(args, sig)]
        return fn(*cast)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# vit.hip
# ------------------------------------------------------------------------------------------------------------------------------------------------
entry("pf_patch_im2col", dict(B=1, H=14, W=14, ld=588, dtype=0), dict(img=4, out=4),
      {"B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "H%14": dict(H=15), "W%14": dict(W=13), "ld<588": dict(ld=587), "dtype=9": dict(dtype=9),
       "dtype=-1": dict(dtype=-1)},
      corners=("patch_im2col",))
entry("pf_assemble_tokens", dict(B=1, S=2, D=8, dtype=0), dict(emb=4, tokens=4, cls=4, pos=4),
      {"B=0": dict(B=0), "S=0": dict(S=0), "D=0": dict(D=0), "D=6": dict(D=6), "D=-8": dict(D=-8), "dtype=5": dict(dtype=5)},
      corners=("assemble_tokens",))
entry("pf_layernorm", dict(x_ld=32, y_ld=32, eps=1e-6, batches=1, in_rows_per_batch=4, in_row_offset=0, out_rows_per_batch=4, D=32, dtype=0),
      dict(x=16, y=16, g=4, b=4),
      {"y_ld<D": dict(y_ld=8), "x_ld<D": dict(x_ld=8), "x_ld%8": dict(x_ld=36), "y_ld%8": dict(y_ld=36), "D=0": dict(D=0), "D%8": dict(D=12, x_ld=16, y_ld=16),
       "D=2056": dict(D=2056, x_ld=2056, y_ld=2056), "remap past the batch": dict(in_row_offset=2), "in_row_offset<0": dict(in_row_offset=-1),
       "batches=0": dict(batches=0), "out_rows=0": dict(out_rows_per_batch=0), "in_rows=0": dict(in_rows_per_batch=0, out_rows_per_batch=0),
       "rows=2^31": dict(batches=1 << 16, out_rows_per_batch=1 << 15, in_rows_per_batch=1 << 15), "dtype=7": dict(dtype=7)},
      corners=("layernorm",))
entry("pf_qkv_split", dict(B=1, S=5, Hh=1, Sp=64, scale=0.125, dtype=0), dict(qkv=16, q=16, k=16, vt=16),
      {"B=0": dict(B=0), "S=0": dict(S=0), "Hh=0": dict(Hh=0), "Sp%64": dict(Sp=65), "Sp<S": dict(S=65), "B*Hh=65536": dict(B=256, Hh=256), "dtype=5": dict(dtype=5)},
      corners=("vit_attention_heads",))
entry("pf_vit_attention", dict(B=1, S=5, Sp=64, Hh=1, dtype=0), dict(q=16, k=16, vt=16, out=16),
      {"B=0": dict(B=0), "S=0": dict(S=0), "Hh=0": dict(Hh=0), "Sp%64": dict(Sp=65), "Sp<S": dict(S=65), "B*Hh=65536": dict(B=256, Hh=256), "dtype=5": dict(dtype=5)},
      corners=("vit_attention_heads",))
entry("pf_vit_attention_rpb_bf16_lds_bytes", dict(S=5, th=1, tw=4), {},
      {"S!=th*tw+1": dict(S=6), "tw<4": dict(S=4, tw=3), "th=0": dict(th=0, S=1), "S=2^20": dict(S=1 << 20, th=1, tw=(1 << 20) - 1)}, no=-1, query=True)
entry("pf_vit_attention_rpb_bf16", dict(B=1, S=5, Sp=64, Hh=1, th=1, tw=4), dict(q=16, k=16, vt=16, out=8, tab=4),
      {"B=0": dict(B=0), "Hh=0": dict(Hh=0), "S!=th*tw+1": dict(S=6), "tw<4": dict(S=4, tw=3), "th=0": dict(th=0, S=1), "Sp%64": dict(Sp=72),
       "Sp<S": dict(S=129, th=32, tw=4), "B*Hh=65536": dict(B=256, Hh=256), "S=2^20": dict(S=1 << 20, th=1, tw=(1 << 20) - 1, Sp=1 << 20),
       "table slice above the LDS": dict(S=200 * 200 + 1, th=200, tw=200, Sp=40064)},
      corners=("vit_attention_rpb_bf16",))
entry("pf_vit_attention_qkv", dict(B=1, S=5, Hh=1, dtype=0), dict(qkv=16, out=16),
      {"B=0": dict(B=0), "S=0": dict(S=0), "Hh=0": dict(Hh=0), "dtype=1": dict(dtype=1), "B*Hh=65536": dict(B=256, Hh=256)},
      corners=("vit_attention_qkv",))
entry("pf_vit_attention_qkv_split3", dict(plane=320, kmajor=0, B=1, S=5, Hh=1), dict(qkv=16, out3=8),
      {"B=0": dict(B=0), "S=0": dict(S=0), "Hh=0": dict(Hh=0), "plane<B*S*D": dict(plane=316), "plane%4": dict(plane=322), "B*Hh=65536": dict(B=256, Hh=256, plane=1 << 40)},
      corners=("vit_attention_qkv_split3",))
entry("pf_layernorm_split3", dict(x_ld=32, y_ld=32, plane=128, kmajor=0, eps=1e-6, rows=4, D=32), dict(x=16, y3=8, g=4, b=4),
      {"x_ld<D": dict(x_ld=8), "y_ld<D": dict(y_ld=8), "x_ld%8": dict(x_ld=36), "y_ld%8": dict(y_ld=36, plane=256), "D=0": dict(D=0), "D%8": dict(D=12),
       "D=2056": dict(D=2056, x_ld=2056, y_ld=2056, plane=1 << 20), "rows=0": dict(rows=0), "rows=2^31": dict(rows=1 << 31, plane=1 << 40),
       "plane below the rows": dict(plane=124), "plane%4": dict(plane=130), "kmajor: D%32": dict(kmajor=1, D=8, x_ld=8, y_ld=8),
       "kmajor: y_ld!=D": dict(kmajor=1, y_ld=40, plane=256)},
      corners=("layernorm_planes",))
entry("pf_layernorm_f16x2", dict(x_ld=32, eps=1e-6, rows=4, D=32), dict(x=16, y2=16, in_exp=4, g=4, b=4),
      {"x_ld<D": dict(x_ld=24), "x_ld%8": dict(x_ld=36), "D=0": dict(D=0), "D%32": dict(D=16), "D=2080": dict(D=2080, x_ld=2080), "rows=0": dict(rows=0),
       "rows=2^31": dict(rows=1 << 31)},
      corners=("layernorm_planes",))
entry("pf_vit_attention_split3", dict(plane_in=960, plane_out=320, kmajor=0, B=1, S=5, Hh=1), dict(qkv3=16, out3=8),
      {"B=0": dict(B=0), "S=0": dict(S=0), "Hh=0": dict(Hh=0), "plane_in short": dict(plane_in=952), "plane_out short": dict(plane_out=316),
       "plane_in%8": dict(plane_in=964), "plane_out%4": dict(plane_out=322), "B*Hh=65536": dict(B=256, Hh=256, plane_in=1 << 28, plane_out=1 << 28),
       "32-bit tile offsets": dict(plane_in=1 << 31, plane_out=1 << 31)},
      corners=("vit_attention_split3",))

# ------------------------------------------------------------------------------------------------------------------------------------------------
# attn_split3.hip
# ------------------------------------------------------------------------------------------------------------------------------------------------
_ATTN3 = {"B=0": dict(B=0), "S=0": dict(S=0), "Hh=0": dict(Hh=0), "plane_in short": dict(plane_in=952), "plane_out short": dict(plane_out=316),
          "plane_in%8": dict(plane_in=964), "plane_out%4": dict(plane_out=322),
          "S*Hh*384>=2^31": dict(S=1 << 19, Hh=11, plane_in=1 << 40, plane_out=1 << 40)}
entry("pf_vit_attention_split3_v2", dict(plane_in=960, plane_out=320, kmajor=0, B=1, S=5, Hh=1, queries_per_wave=0, schedule=0), dict(qkv3=16, out3=8),
      dict(_ATTN3, **{"queries_per_wave=8": dict(queries_per_wave=8), "schedule=3": dict(schedule=3), "schedule=-1": dict(schedule=-1)}),
      corners=("vit_attention_split3_v2",))
entry("pf_vit_attention_f16x2", dict(plane_in=960, plane_out=320, B=1, S=5, Hh=1), dict(qkv2=16, qk_exp=4, out=8, v_exp3=16), dict(_ATTN3),
      optional=("v_exp3",), corners=("vit_attention_f16x2",))
entry("pf_vit_attention_split3_rpb", dict(plane_in=960, plane_out=320, kmajor=0, B=1, S=5, Hh=1, th=1, tw=4, queries_per_wave=0), dict(qkv3=16, out3=8, tab=4),
      dict({k: v for k, v in _ATTN3.items() if k not in ("S=0", "S*Hh*384>=2^31")},
           **{"S!=th*tw+1": dict(S=6, plane_in=1 << 20, plane_out=1 << 20), "th=0": dict(th=0), "tw=0": dict(tw=0), "queries_per_wave=8": dict(queries_per_wave=8),
              "S=2^20": dict(S=1 << 20, th=1, tw=(1 << 20) - 1, plane_in=1 << 40, plane_out=1 << 40),
              "table slice above the LDS": dict(S=200 * 200 + 1, th=200, tw=200, plane_in=1 << 30, plane_out=1 << 30)}),
      corners=("vit_attention_split3_rpb",))

# ------------------------------------------------------------------------------------------------------------------------------------------------
# beit.hip, beit_bf16.hip (mean3 / std3 are HOST arrays: the launcher reads them)
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _f3(*v):
    return (C.c_float * 3)(*v)


_IM2COL_NORM = {"B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "patch=0": dict(patch=0), "H%patch": dict(H=17), "W%patch": dict(W=15),
                "ld<3*patch^2": dict(ld=767), "std=0": dict(std3=_f3(0.5, 0.0, 0.5)), "std=nan": dict(std3=_f3(0.5, float("nan"), 0.5))}
entry("pf_patch_im2col_norm", dict(B=1, H=16, W=16, patch=16, mean3=_f3(0.5, 0.5, 0.5), std3=_f3(0.5, 0.5, 0.5), ld=768), dict(img=4, out=4, mean3="host", std3="host"),
      dict(_IM2COL_NORM), corners=("patch_im2col_norm",))
entry("pf_patch_im2col_norm_bf16", dict(B=1, H=16, W=16, patch=16, mean3=_f3(0.5, 0.5, 0.5), std3=_f3(0.5, 0.5, 0.5), ld=768),
      dict(img=4, out=2, mean3="host", std3="host"), dict(_IM2COL_NORM), corners=("patch_im2col_norm",))
entry("pf_readout_concat", dict(x_ld=4, B=1, S=2, D=4, y_ld=8), dict(x=16, y=16),
      {"B=0": dict(B=0), "S=1": dict(S=1), "D=0": dict(D=0), "D%4": dict(D=2), "x_ld<D": dict(D=8, y_ld=16), "y_ld<2D": dict(y_ld=4), "x_ld%4": dict(x_ld=6),
       "y_ld%4": dict(y_ld=10)}, corners=("readout_concat",))
entry("pf_readout_concat_bf16", dict(x_ld=8, B=1, S=2, D=8, y_ld=16), dict(x=16, y=16),
      {"B=0": dict(B=0), "S=1": dict(S=1), "D=0": dict(D=0), "D%8": dict(D=4), "x_ld<D": dict(D=16, y_ld=32), "y_ld<2D": dict(y_ld=8), "x_ld%8": dict(x_ld=12),
       "y_ld%8": dict(y_ld=20)}, corners=("readout_concat",))

# ------------------------------------------------------------------------------------------------------------------------------------------------
# swin.hip
# ------------------------------------------------------------------------------------------------------------------------------------------------
entry("pf_swin_ln_partition", dict(x_ld=8, eps=1e-5, B=1, H=1, W=1, C=8, shift=0, dtype=0), dict(x=16, xw=16, g=4, b=4),
      {"B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "C=0": dict(C=0), "C%8": dict(C=12, x_ld=16), "C/8 not a power of two": dict(C=24, x_ld=24),
       "C=1024": dict(C=1024, x_ld=1024), "x_ld<C": dict(C=16), "x_ld%8": dict(x_ld=12), "shift=-1": dict(shift=-1), "shift=12": dict(shift=12),
       "dtype=2": dict(dtype=2), "tokens=2^31": dict(B=1 << 12, H=720, W=732)},
      corners=("swin",))
entry("pf_swin_window_attention", dict(B=1, Hp=12, Wp=12, C=8, heads=1, shift=0, dtype=0), dict(qkv=16, out=16, bias_table=4),
      {"heads=0": dict(heads=0), "heads=-1": dict(heads=-1), "C%heads": dict(heads=3), "head_dim=1": dict(heads=8), "head_dim=64": dict(C=64), "B=0": dict(B=0),
       "Hp=0": dict(Hp=0), "Hp%12": dict(Hp=13), "Wp%12": dict(Wp=18), "C=0": dict(C=0), "C%8": dict(C=4, heads=2), "shift=12": dict(shift=12),
       "shift=-6": dict(shift=-6), "dtype=3": dict(dtype=3), "heads=65536": dict(C=131072, heads=65536)},
      corners=("swin",))
entry("pf_swin_unpartition_add", dict(s_ld=8, y_ld=8, B=1, H=1, W=1, C=8, shift=0, dtype=0), dict(proj=16, shortcut=16, y=16),
      {"B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "C=0": dict(C=0), "C%8": dict(C=4), "s_ld<C": dict(s_ld=0), "y_ld<C": dict(C=16, s_ld=16),
       "s_ld%8": dict(s_ld=12), "y_ld%8": dict(y_ld=12), "shift=12": dict(shift=12), "shift=-1": dict(shift=-1), "dtype=2": dict(dtype=2)},
      corners=("swin",))
entry("pf_add_rowwise", dict(x_ld=8, B=1, T=1, C=8, dtype=0), dict(x=16, pos=4),
      {"B=0": dict(B=0), "T=0": dict(T=0), "C=0": dict(C=0), "C%8": dict(C=12, x_ld=16), "x_ld<C": dict(C=16), "x_ld%8": dict(x_ld=12), "dtype=2": dict(dtype=2)},
      corners=("add_rowwise",))

# ------------------------------------------------------------------------------------------------------------------------------------------------
# imageops.hip
# ------------------------------------------------------------------------------------------------------------------------------------------------
_RESIZE = {"B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "C=0": dict(C=0), "C%8": dict(C=12, x_ld=16, y_ld=16), "OH=0": dict(OH=0), "OW=0": dict(OW=0),
           "x_ld<C": dict(x_ld=0), "y_ld<C": dict(C=16, x_ld=16), "x_ld%8": dict(x_ld=12), "y_ld%8": dict(y_ld=12), "dtype=4": dict(dtype=4),
           "add_ld<C": dict(add=0x7f000000, add_ld=0), "add_ld%8": dict(add=0x7f000000, add_ld=12), "B*OH=2^31": dict(B=1 << 16, OH=1 << 15)}
entry("pf_resize_bilinear", dict(x_ld=8, B=1, H=1, W=1, C=8, y_ld=8, OH=3, OW=5, add=None, add_ld=0, in_f32=1, out_f32=1, dtype=0), dict(x=16, y=16, add=16),
      dict(_RESIZE), optional=("add",), corners=("resize",))
entry("pf_resize_bilinear_ex", dict(x_ld=8, B=1, H=1, W=1, C=8, y_ld=8, OH=3, OW=5, add=None, add_ld=0, in_f32=1, out_f32=1, dtype=0), dict(x=16, y=16, add=16, cmax=4),
      dict(_RESIZE, **{"maxima with bf16": dict(dtype=1, in_f32=0, out_f32=0, cmax=0x7b000000)}), optional=("add", "cmax"), corners=("resize",))


def _concat_good(lds=(8, 8), Hs=(1, 1), Ws=(1, 1), Cs=(8, 8), srcs=(0x7e000000, 0x7e100000)):
    n = len(lds)
    arr = lambda v: (C.c_int * n)(*v)
    return dict(xs=(C.c_void_p * n)(*srcs), lds=arr(lds), Hs=arr(Hs), Ws=arr(Ws), Cs=arr(Cs))


_CONCAT = {"nsrc=1": dict(nsrc=1), "nsrc=4": dict(nsrc=4), "B=0": dict(B=0), "OH=0": dict(OH=0), "OW=0": dict(OW=0), "y_ld%8": dict(y_ld=20), "y_ld<sum C": dict(y_ld=8),
           "dtype=2": dict(dtype=2), "a null source": _concat_good(srcs=(0x7e000000, None)), "a misaligned source": _concat_good(srcs=(0x7e000000, 0x7e100008)),
           "C%8": _concat_good(Cs=(8, 4)), "C=0": _concat_good(Cs=(8, 0)), "ld%8": _concat_good(lds=(8, 12)), "ld<C": _concat_good(lds=(8, 0)),
           "H=0": _concat_good(Hs=(0, 1)), "W=0": _concat_good(Ws=(1, 0))}
_CONCAT_PTRS = dict(xs="host", lds="host", Hs="host", Ws="host", Cs="host", y=16)
entry("pf_resize_concat", dict(_concat_good(), nsrc=2, B=1, y_ld=16, OH=3, OW=5, dtype=0), dict(_CONCAT_PTRS), dict(_CONCAT), corners=("resize",))
entry("pf_resize_concat_ex", dict(_concat_good(), nsrc=2, B=1, y_ld=16, OH=3, OW=5, dtype=0), dict(_CONCAT_PTRS, cmax=4),
      dict(_CONCAT, **{"maxima with bf16": dict(dtype=1, cmax=0x7b000000)}), optional=("cmax",), corners=("resize",))
entry("pf_crop_resize_planar", dict(C=3, H=4, W=4, P=1, oh=2, ow=2), dict(img=4, boxes=4, out=4),
      {"C=0": dict(C=0), "H=0": dict(H=0), "W=0": dict(W=0), "P=0": dict(P=0), "oh=0": dict(oh=0), "ow=0": dict(ow=0), "P*4=2^31": dict(P=1 << 29)},
      no_corner="the boxes live on the device and the engine's crops are whole tiles: tests/test_image_grade_gpu.py test_crop_resize grades the edge boxes")
_ROI = {"Bf=0": dict(Bf=0), "H=0": dict(H=0), "W=0": dict(W=0), "C=0": dict(C=0), "C%8": dict(C=12, f_ld=16, y_ld=16), "K=0": dict(K=0), "oh=0": dict(oh=0),
        "ow=0": dict(ow=0), "f_ld<C": dict(f_ld=0), "y_ld<C": dict(y_ld=0), "f_ld%8": dict(f_ld=12), "y_ld%8": dict(y_ld=12), "dtype=2": dict(dtype=2),
        "spatial_scale=0": dict(spatial_scale=0.0), "C=1 with bf16 storage": dict(C=1, f_ld=1, y_ld=1, in_f32=0), "K*oh=2^31": dict(K=1 << 16, oh=1 << 15)}
entry("pf_roi_align", dict(f_ld=8, Bf=1, H=2, W=2, C=8, K=1, y_ld=8, oh=2, ow=2, spatial_scale=1.0, in_f32=1, out_f32=1, dtype=0), dict(feat=16, rois=4, y=16),
      dict(_ROI), corners=("roi_align",))
entry("pf_roi_align_ex", dict(f_ld=8, Bf=1, H=2, W=2, C=8, K=1, y_ld=8, oh=2, ow=2, spatial_scale=1.0, in_f32=1, out_f32=1, dtype=0), dict(feat=16, rois=4, y=16, cmax=4),
      dict(_ROI, **{"maxima with bf16": dict(dtype=1, in_f32=0, out_f32=0, cmax=0x7b000000), "maxima of the planar map": dict(C=1, f_ld=1, y_ld=1, cmax=0x7b000000),
                    "maxima: C=8200": dict(C=8200, f_ld=8200, y_ld=8200, cmax=0x7b000000)}), optional=("cmax",), corners=("roi_align",))
entry("pf_maxpool2", dict(x_ld=8, B=1, H=2, W=2, C=8, y_ld=8, dtype=0), dict(x=16, y=16),
      {"B=0": dict(B=0), "H=1": dict(H=1), "W=1": dict(W=1), "C=0": dict(C=0), "C%8": dict(C=12, x_ld=16, y_ld=16), "x_ld<C": dict(x_ld=0), "y_ld<C": dict(y_ld=0),
       "x_ld%8": dict(x_ld=12), "y_ld%8": dict(y_ld=12), "dtype=2": dict(dtype=2)}, corners=("maxpool2",))
_COPY = {"npix=0": dict(npix=0), "npix<0": dict(npix=-4), "C=0": dict(C=0), "C%8": dict(C=12, x_ld=16, y_ld=16), "x_ld<C": dict(x_ld=0), "y_ld<C": dict(y_ld=0),
         "x_ld%8": dict(x_ld=12), "y_ld%8": dict(y_ld=12), "dtype=2": dict(dtype=2)}
entry("pf_copy_channels", dict(x_ld=8, y_ld=8, npix=1, C=8, in_f32=1, out_f32=1, dtype=0), dict(x=16, y=16), dict(_COPY), corners=("copy_channels",))
entry("pf_copy_channels_ex", dict(x_ld=8, y_ld=8, npix=1, C=8, in_f32=1, out_f32=1, dtype=0), dict(x=16, y=16, cmax=4),
      dict(_COPY, **{"maxima with bf16": dict(dtype=1, in_f32=0, out_f32=0, cmax=0x7b000000), "maxima: C=8200": dict(C=8200, x_ld=8200, y_ld=8200, cmax=0x7b000000)}), optional=("cmax",),
      corners=("copy_channels",))
entry("pf_zero_u32", dict(n=4), dict(p=4), {"n=0": dict(n=0), "n<0": dict(n=-1)}, no_corner="a memset: tests/test_cmax_producers_gpu.py runs it before every producer")
entry("pf_pack_fusion_input", dict(B=1, h=1, w=1, dtype=0), dict(cdepth=4, fdepth=4, crops=4, y=16),
      {"B=0": dict(B=0), "h=0": dict(h=0), "w=0": dict(w=0), "dtype=2": dict(dtype=2)}, corners=("pack_fusion_input",))
entry("pf_nhwc_to_nchw_f32", dict(x_ld=8, B=1, H=1, W=1, C=8, in_f32=1, dtype=0), dict(x=4, y=4),
      {"B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "C=0": dict(C=0), "x_ld<C": dict(x_ld=4), "dtype=2": dict(dtype=2)}, corners=("nhwc_to_nchw",))
entry("pf_attractor", dict(a_ld=1, n_attr=1, a_stride=1, a_eps=0.0, attractor_exp=0, kind_sum=0, hp=1, wp=1, B=1, h=1, w=1, n_bins=4), dict(A=4, b_prev=16, out=16),
      {"n_bins=0": dict(n_bins=0), "n_bins%4": dict(n_bins=6), "n_attr=0": dict(n_attr=0), "a_stride=0": dict(a_stride=0), "a_ld below the attractors": dict(n_attr=2), "a_ld=0": dict(a_ld=0),
       "B=0": dict(B=0), "h=0": dict(h=0), "w=0": dict(w=0), "hp=0": dict(hp=0), "wp=0": dict(wp=0)}, corners=("bins",))
entry("pf_seed_bin_centers", dict(x_ld=4, npix=1, n_bins=4, min_depth=1e-3, max_depth=10.0, bounded=1, normalize=0), dict(x=4, out=4),
      {"npix=0": dict(npix=0), "n_bins=0": dict(n_bins=0), "x_ld<n_bins": dict(x_ld=3)}, corners=("bins",))
entry("pf_bounded_bin_centers", dict(npix=1, n_bins=4, min_depth=1e-3, max_depth=10.0), dict(b=4, out=4),
      {"npix=0": dict(npix=0), "n_bins=0": dict(n_bins=0), "n_bins=65": dict(n_bins=65)}, corners=("bins",))
entry("pf_logbinom_depth", dict(pt_ld=4, hc=1, wc=1, B=1, h=1, w=1, n_bins=4, min_temp=0.0212, max_temp=50.0), dict(pt=4, centers=16, depth=4),
      {"n_bins=0": dict(n_bins=0), "n_bins%4": dict(n_bins=6), "n_bins=260": dict(n_bins=260), "pt_ld<4": dict(pt_ld=3), "B=0": dict(B=0), "h=0": dict(h=0),
       "w=0": dict(w=0), "hc=0": dict(hc=0), "wc=0": dict(wc=0)}, corners=("bins",))
entry("pf_stitch_init", dict(MH=2, MW=2, P=1, ph=1, pw=1), dict(pred=4, count=4, depth=4, mask=4, yx=4),
      {"MH=0": dict(MH=0), "MW=0": dict(MW=0), "P=0": dict(P=0), "ph=0": dict(ph=0), "pw=0": dict(pw=0), "P*2=2^31": dict(P=1 << 30)},
      no_corner="the tile origins live on the device; tests/test_image_grade_gpu.py test_stitch grades the tiles at the far edges")
entry("pf_stitch_finish_init", dict(n=1), dict(avg=4, pred=4, count=4), {"n=0": dict(n=0), "n<0": dict(n=-1)},
      no_corner="an element-wise quotient without shape arguments: tests/test_image_grade_gpu.py test_stitch")
entry("pf_stitch_update", dict(MH=4, MW=4, dh=2, dw=2, y0=2, x0=2, ph=2, pw=2), dict(avg=4, count=4, depth=4, mask=4),
      {"y0<0": dict(y0=-1), "x0<0": dict(x0=-1), "y0=MH": dict(y0=4), "x0=MW": dict(x0=4), "MH=0": dict(MH=0), "MW=0": dict(MW=0), "dh=0": dict(dh=0), "dw=0": dict(dw=0),
       "ph=0": dict(ph=0), "pw=0": dict(pw=0)}, corners=("stitch_update",))
_PLANE = {"H=0": dict(H=0), "W=0": dict(W=0), "OH=0": dict(OH=0), "OW=0": dict(OW=0)}
entry("pf_resize_nearest_f32", dict(H=1, W=1, OH=3, OW=5), dict(x=4, y=4), dict(_PLANE), corners=("planar_resize",))
entry("pf_resize_bilinear_f32", dict(H=1, W=1, OH=3, OW=5), dict(x=4, y=4), dict(_PLANE), corners=("planar_resize",))
entry("pf_bins_tail", dict(clb_ld=32, rel_off=0, he=1, we=1, hc=1, wc=1, B=1, H=1, W=1, nq=10, min_temp=0.0212, max_temp=50.0),
      dict(clb=16, emb=16, w0f=16, b0=4, w2=4, b2=4, centers=16, depth=4),
      {"clb_ld<32": dict(clb_ld=28), "clb_ld%4": dict(clb_ld=34), "nq=9": dict(nq=9), "nq=12": dict(nq=12), "rel slice outside the row": dict(nq=11, rel_off=28),
       "rel_off%4": dict(nq=11, rel_off=2, clb_ld=48), "rel_off<0": dict(nq=11, rel_off=-4), "B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "he=0": dict(he=0),
       "we=0": dict(we=0), "hc=0": dict(hc=0), "wc=0": dict(wc=0)},
      no_corner="its one-pixel map is a case of tests/test_tail_grade_gpu.py (the fused tail's own grade module)")

# ------------------------------------------------------------------------------------------------------------------------------------------------
# pf_conv_params entry points: igemm.hip, gemm_split3.hip, conv1x1_split3.hip, wino*.hip, gemm_f16x2_t160.hip (reached through pf_gemm_f16x2)
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _pp(**kw):
    return {f"p.{k}": v for k, v in kw.items()}


_CONV_GOOD = _pp(x_ld=4, B=1, H=1, W=1, Cin=4, w_rows=4, Kpad=32, y_ld=4, OH=1, OW=1, Cout=4, KH=1, KW=1, stride=1, pad=0, act=0, relu_in=0, out_f32=0, shuffle=1,
                 dtype=0, korder=0, batch=0)
_CONV_PTRS = {"p.x": 16, "p.w": 16, "p.y": 16, "p.bias": 4, "p.scale": 4, "p.res": 4, "p.res2": 4}
_RES = {"p.res": 0x7d000000, "p.res_ld": 4}
_CONV = {"y_ld<Cout": _pp(y_ld=0), "res_ld<Cout": dict(_RES, **_pp(res_ld=0)), "res2_ld<Cout": {"p.res2": 0x7d000000, "p.res2_ld": 0}, "y_ld%4": _pp(y_ld=6),
         "res_ld%4": dict(_RES, **_pp(res_ld=6)), "res2_ld%4": {"p.res2": 0x7d000000, "p.res2_ld": 6}, "stride=0": _pp(stride=0), "pad=-1": _pp(pad=-1, KH=1),
         "shuffle=0": _pp(shuffle=0), "shuffle=-2": _pp(shuffle=-2), "act=99": _pp(act=99), "act=-1": _pp(act=-1), "OH unrelated": _pp(OH=3), "OW unrelated": _pp(OW=2),
         "B=0": _pp(B=0), "H=0": _pp(H=0), "W=0": _pp(W=0), "KH=0": _pp(KH=0), "KW=0": _pp(KW=0), "filter above the padded input": _pp(KH=3, KW=3),
         "17 taps": _pp(KH=17, H=17, Kpad=96), "Cin=0": _pp(Cin=0), "Cin%4": _pp(Cin=6, x_ld=8), "x_ld<Cin": _pp(x_ld=0), "x_ld%4": _pp(x_ld=6), "Cout=0": _pp(Cout=0),
         "Cout%4": _pp(Cout=6, y_ld=8, w_rows=8), "w_rows<Cout": _pp(w_rows=0), "Kpad%32": _pp(Kpad=40), "Kpad=0": _pp(Kpad=0), "Kpad<KH*KW*Cin": _pp(Cin=64, x_ld=64),
         "dtype=2": _pp(dtype=2), "korder=2": _pp(korder=2), "korder=1 with Cin%32": _pp(korder=1), "batch<0": _pp(batch=-1),
         "batch=65536": _pp(batch=65536, x_bstride=4, w_bstride=128, y_bstride=4), "batch without strides": _pp(batch=2),
         "batch with a bias": dict({"p.bias": 0x7d000000}, **_pp(batch=2, x_bstride=4, w_bstride=128, y_bstride=4)),
         "B*OH*OW=2^31": _pp(B=1 << 15, H=1 << 8, W=1 << 8, OH=1 << 8, OW=1 << 8), "shuffle: Cout/s^2 % 4": _pp(shuffle=2, Cout=8, w_rows=8, y_ld=8),
         "shuffle with 3x3": _pp(shuffle=2, Cout=16, w_rows=16, y_ld=4, KH=3, KW=3, pad=1, Kpad=64), "bf16: Cin%8": _pp(dtype=1, Kpad=64)}
_CONV_CORNERS = ("conv",)
entry("pf_conv", dict(_CONV_GOOD), dict(_CONV_PTRS), dict(_CONV, **{"null p": dict(p="NULL")}), optional=("p.bias", "p.scale", "p.res", "p.res2"),
      corners=_CONV_CORNERS, reads=set(CONV_INT_FIELDS) - {"x_bstride", "w_bstride", "y_bstride"} | {"x_bstride"})
entry("pf_conv_timed", dict(_CONV_GOOD, iters=1, ms=(C.c_float * 1)(0.0)), dict(_CONV_PTRS, ms="host"),
      dict({k: v for k, v in _CONV.items() if k in ("y_ld<Cout", "stride=0", "shuffle=0", "act=99", "OH unrelated", "dtype=2", "Cin%4")},
           **{"iters=0": dict(iters=0), "null p": dict(p="NULL")}),
      optional=("p.bias", "p.scale", "p.res", "p.res2"), no_corner="pf_conv between two HIP events: the timing helper of bench.py's roofline entry", reads={"stride"})

# the linear family: M = B * OH * OW rows of a 1 x 1 layer
_LIN_GOOD = _pp(x_ld=32, B=1, H=1, W=4, Cin=32, w_rows=16, Kpad=32, y_ld=16, OH=1, OW=4, Cout=16, KH=1, KW=1, stride=1, pad=0, act=0, relu_in=0, out_f32=1, shuffle=1,
                dtype=1, korder=0, batch=0, x_bstride=128, w_bstride=512, y_bstride=64)
_LIN = {"KH=3": _pp(KH=3), "KW=3": _pp(KW=3), "stride=2": _pp(stride=2), "pad=1": _pp(pad=1), "shuffle=0": _pp(shuffle=0), "shuffle=2": _pp(shuffle=2), "act=99": _pp(act=99),
        "act=-1": _pp(act=-1), "B=0": _pp(B=0), "H!=OH": _pp(H=2), "W!=OW": _pp(W=5), "OH=0": _pp(OH=0, H=0), "OW=0": _pp(OW=0, W=0), "batch<0": _pp(batch=-1),
        "batch=65536": _pp(batch=65536), "Cin=0": _pp(Cin=0), "Cin%32": _pp(Cin=16), "x_ld<Cin": _pp(x_ld=24), "Cout=0": _pp(Cout=0), "Cout%4": _pp(Cout=6),
        "y_ld<Cout": _pp(y_ld=12), "y_ld%4": _pp(y_ld=18), "w_rows<Cout": _pp(w_rows=12), "res_ld<Cout": {"p.res": 0x7d000000, "p.res_ld": 12},
        "res_ld%4": {"p.res": 0x7d000000, "p.res_ld": 18}, "res2_ld<Cout": {"p.res2": 0x7d000000, "p.res2_ld": 12}, "null p": dict(p="NULL")}
_S3 = dict(_LIN, **{"Kpad<Cin": _pp(Kpad=0), "Kpad%32": _pp(Kpad=40), "x_ld%8": _pp(x_ld=36), "x_bstride=0": _pp(x_bstride=0), "w_bstride=0": _pp(w_bstride=0),
                    "x_bstride%8": _pp(x_bstride=132), "w_bstride%8": _pp(w_bstride=516), "plane output without y_bstride": _pp(out_f32=0, y_bstride=0),
                    "y_bstride%4": _pp(out_f32=0, y_bstride=66), "korder=1": _pp(korder=1), "korder=16": _pp(korder=16), "chunk-major x with a padded row": _pp(korder=2, x_ld=40),
                    "chunk-major w with padded K": _pp(korder=4, Kpad=64), "chunk-major y as float32": _pp(korder=8), "chunk-major y with Cout%32": _pp(korder=8, out_f32=0),
                    "batch with a bias": dict({"p.bias": 0x7d000000}, **_pp(batch=2)), "batch with plane output": _pp(batch=2, out_f32=0),
                    "M=2^31": _pp(B=1 << 15, H=1 << 8, W=1 << 8, OH=1 << 8, OW=1 << 8)})
_S3_PTRS = {"p.x": 16, "p.w": 16, "p.y": 16, "p.bias": 16, "p.scale": 16, "p.res": 16, "p.res2": 16}
_S3_OPT = ("p.bias", "p.scale", "p.res", "p.res2")
_S3_READS = set(CONV_INT_FIELDS) - {"dtype", "relu_in"}
entry("pf_gemm_split3", dict(_LIN_GOOD), dict(_S3_PTRS), dict(_S3), optional=_S3_OPT, corners=("linears",), reads=_S3_READS)
entry("pf_gemm_split3_ex", dict(_LIN_GOOD, grid_cap=0), dict(_S3_PTRS), dict(_S3), optional=_S3_OPT, corners=("linears",), reads=_S3_READS)
entry("pf_gemm_split3_timed", dict(_LIN_GOOD, iters=1, ms=(C.c_float * 1)(0.0)), dict(_S3_PTRS, ms="host"),
      dict({k: v for k, v in _S3.items() if k in ("KH=3", "Cin%32", "y_ld<Cout", "act=99", "null p")}, **{"iters=0": dict(iters=0)}), optional=_S3_OPT,
      no_corner="pf_gemm_split3 between two HIP events: the timing helper of bench.py's roofline entry", reads={"KH"})
_PTS_GOOD = dict(_LIN_GOOD, **_pp(korder=6, batch=36, x_bstride=36 * 128, w_bstride=36 * 512, w_rows=16))      # (the persistent walk wants 8 tiles: 36 transform points)
_PTS = dict({k: v for k, v in _LIN.items()},
            **{"korder=0": _pp(korder=0), "float32 output only": _pp(out_f32=0), "x_ld!=Cin": _pp(x_ld=40), "Kpad!=Cin": _pp(Kpad=64), "w_rows%4": _pp(w_rows=18),
               "x_bstride=0": _pp(x_bstride=0), "w_bstride=0": _pp(w_bstride=0), "x_bstride%8": _pp(x_bstride=260), "w_bstride%8": _pp(w_bstride=1028),
               "an epilogue": {"p.bias": 0x7d000000}, "act=1": _pp(act=1), "M*64=2^31": _pp(B=1, H=1, W=1 << 25, OH=1, OW=1 << 25)})
_PTS_PTRS = {"p.x": 16, "p.w": 16, "p.y": 16, "col_exp": 16}
_PTS_READS = set(CONV_INT_FIELDS) - {"dtype", "relu_in", "res_ld", "res2_ld", "y_bstride"} | {"res_ld"}
entry("pf_gemm_f16x2_points", dict(_PTS_GOOD, grid_cap=0), dict(_PTS_PTRS), dict(_PTS), no_corner="not reachable at corner sizes: the fp16x2 product wants two rounds of tiles (pf_conv_winograd_f16x2_supported answers 0, pf_gemm_f16x2_points refuses fewer than 8 tiles); graded by tests/test_wino_f16x2_gpu.py and tests/test_wino_f16x2_n256_gpu.py", reads=_PTS_READS)
entry("pf_gemm_f16x2_points128", dict(_PTS_GOOD, grid_cap=0), dict(_PTS_PTRS), dict(_PTS), no_corner="not reachable at corner sizes: the fp16x2 product wants two rounds of tiles (pf_conv_winograd_f16x2_supported answers 0, pf_gemm_f16x2_points refuses fewer than 8 tiles); graded by tests/test_wino_f16x2_gpu.py and tests/test_wino_f16x2_n256_gpu.py", reads=_PTS_READS)
_F16_GOOD = dict(_LIN_GOOD, **_pp(korder=6, x_bstride=128, w_bstride=512))
_F16 = dict(_LIN, **{"korder=0": _pp(korder=0), "korder bits 16 and 32": _pp(korder=54, out_f32=0), "plane bits with float32 output": _pp(korder=22), "batch=2": _pp(batch=2),
                     "x_ld!=Cin": _pp(x_ld=40), "Kpad!=Cin": _pp(Kpad=64), "w_rows%4": _pp(w_rows=18), "x_bstride=0": _pp(x_bstride=0), "w_bstride=0": _pp(w_bstride=0),
                     "x_bstride%8": _pp(x_bstride=132), "w_bstride%8": _pp(w_bstride=516), "plane output without y_bstride": _pp(out_f32=0, y_bstride=0),
                     "y_bstride%4": _pp(out_f32=0, y_bstride=66), "chunk-major planes without out_exp": _pp(korder=22, out_f32=0, Cout=32, y_ld=32, w_rows=32),
                     "chunk-major planes with Cout%32": dict({"p.out_exp": 0x7d000000}, **_pp(korder=22, out_f32=0)),
                     "row planes without out_exp": _pp(korder=38, out_f32=0), "M*64=2^31": _pp(B=1, H=1, W=1 << 25, OH=1, OW=1 << 25)})
entry("pf_gemm_f16x2", dict(_F16_GOOD), dict(_S3_PTRS, **{"p.col_exp": 16, "p.out_exp": 16}), dict(_F16), optional=_S3_OPT + ("p.out_exp",),
      corners=("linears",), reads=_S3_READS)
_PPG_GOOD = dict(_LIN_GOOD, **_pp(Cin=64, x_ld=64, Kpad=64, out_f32=0))
entry("pf_gemm_bf16_pp", dict(_PPG_GOOD), {"p.x": 16, "p.w": 16, "p.y": 8, "p.bias": 16, "p.scale": 16, "p.res": 8, "p.res2": 8},
      dict({k: v for k, v in _LIN.items() if k not in ("Cin%32", "x_ld<Cin")},
           **{"Cin%64": _pp(Cin=32), "x_ld<Cin": _pp(x_ld=56), "x_ld%8": _pp(x_ld=68), "Kpad<Cin": _pp(Kpad=32), "Kpad%8": _pp(Kpad=68), "dtype=0": _pp(dtype=0),
              "batch=2": _pp(batch=2), "M=2^31": _pp(B=1 << 15, H=1 << 8, W=1 << 8, OH=1 << 8, OW=1 << 8)}),
      optional=_S3_OPT, corners=("gemm_bf16_pp",), reads=set(CONV_INT_FIELDS) - {"relu_in", "korder", "x_bstride", "w_bstride", "y_bstride"})
_C1_GOOD = dict(_LIN_GOOD, **_pp(dtype=0, w_rows=0, Kpad=0, x_bstride=0, w_bstride=0, y_bstride=0), w3_rows=16)
entry("pf_conv1x1_split3", dict(_C1_GOOD), {"p.x": 16, "p.y": 16, "w3": 16, "p.bias": 16, "p.scale": 16, "p.res": 16, "p.res2": 16},
      dict({k: v for k, v in _LIN.items() if k not in ("w_rows<Cout", "batch=65536")},
           **{"dtype=1": _pp(dtype=1), "x_ld%4": _pp(x_ld=34), "w3_rows<Cout": dict(w3_rows=0), "w3_rows%16": dict(w3_rows=24), "batch=2": _pp(batch=2),
              "M=2^31": _pp(B=1 << 15, H=1 << 8, W=1 << 8, OH=1 << 8, OW=1 << 8), "w3_rows*64=2^31": dict(w3_rows=1 << 25)}),
      optional=_S3_OPT, corners=("conv1x1_split3",), reads=set(CONV_INT_FIELDS) - {"w_rows", "Kpad", "korder", "x_bstride", "w_bstride", "y_bstride"})
entry("pf_split3", dict(x_ld=4, y_ld=4, plane=4, rows=1, cols=4), dict(x=16, y=8),
      {"cols=0": dict(cols=0), "cols%4": dict(cols=6, x_ld=8, y_ld=8, plane=8), "x_ld<cols": dict(x_ld=0), "y_ld<cols": dict(y_ld=0), "x_ld%4": dict(x_ld=6),
       "y_ld%4": dict(y_ld=6, plane=8), "rows=0": dict(rows=0), "plane below the rows": dict(plane=0), "plane%4": dict(plane=6)},
      no_corner="the stand-alone split of a float32 matrix: every producer fuses it (the LayerNorm and attention corners grade those stores)")
_ROUTE_GOOD = dict(_LIN_GOOD, **_pp(x_ld=768, W=33152, OW=33152, Cin=768, Cout=768, y_ld=768, w_rows=768, Kpad=768, korder=6, batch=36))   # 768 -> 768 @ 8 x 56 x 74
for _q in ("pf_gemm_split3_route", "pf_gemm_f16x2_points_route", "pf_gemm_f16x2_route"):
    entry(_q, dict(_ROUTE_GOOD, cus=256), {}, {"null p": dict(p="NULL"), "cus=0": dict(cus=0), "cus<0": dict(cus=-8)}, no=-1, query=True)
entry("pf_gemm_f16x2_points_route_ex", dict(_ROUTE_GOOD, cus=256, maxima_given=0), {}, {"null p": dict(p="NULL"), "cus=0": dict(cus=0), "cus<0": dict(cus=-8)}, no=-1,
      query=True)
entry("pf_persist_grid", dict(cus=256, grid_cap=0, total=3672, policy=1 | 2 | 8), {},
      {"cus=0": dict(cus=0), "cus<0": dict(cus=-8), "total=0": dict(total=0), "total<0": dict(total=-8), "total=2^31": dict(total=INT31),
       "no rule below 8 blocks": dict(policy=3), "two rules below 8 blocks": dict(policy=4 | 8), "policy=32": dict(policy=32 | 8),
       "fewer than 8 tiles, refusing": dict(total=7, policy=1 | 16)}, no=-1, query=True)

# the Winograd layers: float32 3 x 3 / stride 1 / pad 1
_W_GOOD = _pp(x_ld=32, B=1, H=4, W=4, Cin=32, y_ld=8, OH=4, OW=4, Cout=8, KH=3, KW=3, stride=1, pad=1, act=0, relu_in=0, out_f32=0, shuffle=1, dtype=0, korder=0, batch=0)
_W = {"dtype=1": _pp(dtype=1), "KH=1": _pp(KH=1), "KW=5": _pp(KW=5), "stride=2": _pp(stride=2), "pad=0": _pp(pad=0), "shuffle=0": _pp(shuffle=0), "shuffle=2": _pp(shuffle=2),
      "a scale": {"p.scale": 0x7d000000}, "B=0": _pp(B=0), "H=0": _pp(H=0, OH=0), "W=0": _pp(W=0, OW=0), "OH!=H": _pp(OH=5), "OW!=W": _pp(OW=3), "Cin=0": _pp(Cin=0),
      "Cin%32": _pp(Cin=48, x_ld=48), "Cout=0": _pp(Cout=0), "Cout%8": _pp(Cout=12, y_ld=12), "x_ld<Cin": _pp(x_ld=24), "y_ld<Cout": _pp(y_ld=4), "x_ld%4": _pp(x_ld=34),
      "y_ld%4": _pp(y_ld=10), "res_ld<Cout": {"p.res": 0x7d000000, "p.res_ld": 4}, "res2_ld%4": {"p.res2": 0x7d000000, "p.res2_ld": 10}, "act=2": _pp(act=2),
      "act=-1": _pp(act=-1), "null p": dict(p="NULL"), "pixels=2^31": _pp(B=1 << 15, H=1 << 8, W=1 << 8, OH=1 << 8, OW=1 << 8)}
_W_PTRS = {"p.x": 16, "p.y": 16, "p.bias": 16, "p.res": 16, "p.res2": 16}
_W_OPT = ("p.bias", "p.res", "p.res2")
_W_READS = set(CONV_INT_FIELDS) - {"w_rows", "Kpad", "relu_in", "out_f32", "korder", "batch", "x_bstride", "w_bstride", "y_bstride"}
entry("pf_conv_winograd", dict(_W_GOOD, m=4, u_rows=8, u_kpad=32), dict(_W_PTRS, U=16, V=16, M=16),
      dict(_W, **{"m=3": dict(m=3), "m=0": dict(m=0), "u_rows<Cout": dict(u_rows=4), "u_kpad<Cin": dict(u_kpad=0), "u_kpad%32": dict(u_kpad=40)}), optional=_W_OPT,
      corners=("winograd", "winograd_abi"), reads=_W_READS)
_W3 = dict(_W, **{"u_rows<Cout": dict(u_rows=0), "u_kpad!=Cin": dict(u_kpad=64)})
_WIN = {"window<0": dict(window=-8), "window%8": dict(window=12)}
entry("pf_conv_winograd_split3", dict(_W_GOOD, u_rows=16, u_kpad=32), dict(_W_PTRS, U3=16, V3=16, M=16), dict(_W3), optional=_W_OPT, corners=("winograd", "winograd_abi"), reads=_W_READS)
entry("pf_conv_winograd_split3_windowed", dict(_W_GOOD, u_rows=16, u_kpad=32, window=0), dict(_W_PTRS, U3=16, V3=16, M=16),
      dict(_W3, **_WIN, **{"x and y overlap across windows": dict({"p.x": 0x60000000, "p.y": 0x60000040}, **_pp(B=1, H=16, W=16, OH=16, OW=16), window=8)}),
      optional=_W_OPT, corners=("winograd", "winograd_abi"), reads=_W_READS)
entry("pf_conv_winograd_split3_windowed_ex", dict(_W_GOOD, u_rows=16, u_kpad=32, window=0, cmax_out=None, cmax_out_relu=0), dict(_W_PTRS, U3=16, V3=16, M=16, cmax_out=4),
      dict(_W3, **_WIN), optional=_W_OPT + ("cmax_out",), corners=("winograd", "winograd_abi"), reads=_W_READS)
_WH = dict(_W, **_WIN, **{"u_rows<Cout": dict(u_rows=0), "u_rows%16": dict(u_rows=24), "u_kpad!=Cin": dict(u_kpad=64), "Cin=8224": _pp(Cin=8224, x_ld=8224)})
entry("pf_conv_winograd_f16x2_windowed", dict(_W_GOOD, u_rows=16, u_kpad=32, window=0), dict(_W_PTRS, U=16, V2=16, M=16, scratch=16), dict(_WH), optional=_W_OPT,
      no_corner="not reachable at corner sizes: the fp16x2 product wants two rounds of tiles (pf_conv_winograd_f16x2_supported answers 0, pf_gemm_f16x2_points refuses fewer than 8 tiles); graded by tests/test_wino_f16x2_gpu.py and tests/test_wino_f16x2_n256_gpu.py", reads=_W_READS)
entry("pf_conv_winograd_f16x2_windowed_ex", dict(_W_GOOD, u_rows=16, u_kpad=32, window=0, cmax_in=None, cmax_out=None, cmax_out_relu=0),
      dict(_W_PTRS, U=16, V2=16, M=16, scratch=16, cmax_in=4, cmax_out=4), dict(_WH, **{"cmax_out is cmax_in": dict(cmax_in=0x7c000000, cmax_out=0x7c000000)}),
      optional=_W_OPT + ("cmax_in", "cmax_out"), no_corner="not reachable at corner sizes: the fp16x2 product wants two rounds of tiles (pf_conv_winograd_f16x2_supported answers 0, pf_gemm_f16x2_points refuses fewer than 8 tiles); graded by tests/test_wino_f16x2_gpu.py and tests/test_wino_f16x2_n256_gpu.py", reads=_W_READS)
_WQ = {k: v for k, v in _WH.items() if k != "pixels=2^31"}
entry("pf_conv_winograd_f16x2_supported", dict(_W_GOOD, **_pp(B=8, H=224, W=296, OH=224, OW=296, Cin=768, x_ld=768, Cout=768, y_ld=768), **{"p.x": 0x50000000, "p.y": 0x58000000}, u_rows=768, u_kpad=768, window=0), {}, dict(_WQ), no=0, query=True)
entry("pf_conv_winograd_f16x2_supported_ex", dict(_W_GOOD, **_pp(B=8, H=224, W=296, OH=224, OW=296, Cin=768, x_ld=768, Cout=768, y_ld=768), **{"p.x": 0x50000000, "p.y": 0x58000000}, u_rows=768, u_kpad=768, window=0, maxima_given=1), {}, dict(_WQ), no=0,
      query=True)
entry("pf_wino_f16x2_scratch_bytes", dict(cin=32, u_rows=16), {}, {"cin=0": dict(cin=0), "u_rows=0": dict(u_rows=0), "cin<0": dict(cin=-32)}, no=0, query=True)
entry("pf_wino_absmax", dict(x_ld=4, P=1, C=4, relu_in=0), dict(x=16, cmax=4),
      {"P=0": dict(P=0), "C=0": dict(C=0), "C%4": dict(C=6, x_ld=8), "x_ld<C": dict(x_ld=0), "x_ld%4": dict(x_ld=6)},
      no_corner="the range pass alone; tests/test_cmax_producers_gpu.py holds every producer to it bit for bit, one-pixel maps included")
_WF_GOOD = dict(_W_GOOD, **_pp(Cout=4, y_ld=4))
_WF = {k: v for k, v in _W.items() if k not in ("Cin%32", "Cout%8", "pixels=2^31")}
_WF.update({"y_ld<Cout": _pp(y_ld=0), "res_ld<Cout": {"p.res": 0x7d000000, "p.res_ld": 0}, "Cin%16": _pp(Cin=40, x_ld=40), "Cin<32": _pp(Cin=16), "Cout%4": _pp(Cout=6, y_ld=8), "B*H*W*x_ld=2^31": _pp(B=1 << 10, H=1 << 8, W=1 << 8, OH=1 << 8, OW=1 << 8)})
entry("pf_conv_winograd_fused_supported", dict(_WF_GOOD, **{"p.x": 0x50000000, "p.y": 0x51000000}), {}, dict(_WF, **{"a misaligned x": {"p.x": 0x50000008}}), no=0, query=True)
entry("pf_conv_winograd_fused", dict(_WF_GOOD, nnb=1, gs=1), dict(_W_PTRS, up=16), dict(_WF, **{"nnb!=ceil(Cout/64)": dict(nnb=2), "nnb=0": dict(nnb=0), "gs<0": dict(gs=-1),
                                                                                              "a forced width of 2": dict(gs=(2 << 16) | 1)}),
      optional=_W_OPT, corners=("winograd",), reads=_W_READS)
entry("pf_conv_winograd_fused_timed", dict(_WF_GOOD, nnb=1, gs=1, iters=1, ms=(C.c_float * 1)(0.0)), dict(_W_PTRS, up=16, ms="host"),
      dict({k: v for k, v in _WF.items() if k in ("dtype=1", "Cin<32", "y_ld<Cout", "null p")}, **{"iters=0": dict(iters=0), "nnb=0": dict(nnb=0), "gs<0": dict(gs=-1)}),
      optional=_W_OPT, no_corner="pf_conv_winograd_fused between two HIP events: a timing helper", reads={"dtype"})
