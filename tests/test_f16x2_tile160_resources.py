"""Build-time guard for the 160 x 256 tile form of the fp16x2 linear (csrc/gemm_f16x2_t160.hip): no scratch, two waves per SIMD, the three-slot ring
as its only LDS (at most 159 744 B), and no vector-memory wait besides vmcnt(0) and the ring's hand-counted ones -- vmcnt(6) in group A (five X
pieces and one W piece per wave and chunk) and vmcnt(7) in group B (seven W pieces)."""
import os
import re

from tests.test_wino_f16x2_resources import _compile, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@needs_hipcc
def test_tile160_gemm_resources_and_waits(tmp_path):
    k = _compile(tmp_path, "gemm_f16x2_t160.hip", ("-save-temps=obj",))
    assert len(k) == 1 and "persist160" in next(iter(k)), list(k)
    (name, (scratch, vgprs, occ)), = k.items()
    assert scratch == 0 and occ >= 2 and vgprs <= 256, (name, scratch, vgprs, occ)
    listing = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    asm = open(tmp_path / listing[0]).read()
    body = asm[asm.index("persist160_kernelE14pf_conv_paramsiii:"):]
    body = body[:body.index(".Lfunc_end")]
    waits = set(re.findall(r"s_waitcnt vmcnt\((\d+)\)", body))
    assert waits <= {"0", "6", "7"}, waits
    assert {"6", "7"} <= waits
    assert body.count("v_mfma_f32_16x16x32_f16") == 120 and "v_mfma_f32_16x16x32_bf16" not in body      # 60 per chunk in each group's loop
    assert "scratch_" not in body and "buffer_store" not in body
    # LDS: none static (.group_segment_fixed_size 0), the launch asks for three stages of 2 x (160 + 256) rows x 64 B
    meta = asm[asm.index(".amdhsa_kernel"):]
    assert re.search(r"\.amdhsa_group_segment_fixed_size 0\b", meta)
    src = open(os.path.join(ROOT, "patchfusion_amd", "csrc", "gemm_f16x2_t160.hip")).read()
    m = re.search(r"constexpr int smem = ([0-9 *()+]+);", src)
    assert m and eval(m.group(1)) == 3 * 53248 <= 159744
    assert "static_assert(" in src and "NS * STAGE <= 159744" in src
