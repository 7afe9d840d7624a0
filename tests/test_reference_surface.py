"""Boundary proof against the reference's REAL surface: the shipped mmengine config files, the
`MODELS.build(cfg.model)` construction path with a ConfigDict (load_branch=True, branch checkpoints from
`pretrain_model`), checkpoint helpers, the HF save/from_pretrained round trip, and `infer_forward` called the way
`BaselinePretrain.regular_tile` calls it (baseline_pretrain.py:293-307).

What the reference itself yields is stored in tests/golden/reference_surface.json (oracle/make_golden.py live): the evaluated `model` dict of
its shipped DA config files, and sha256 digests of its state_dict schema and of its prepare_tile_cfg answers over a seeded sweep of shapes.
The engine is wired to the torch stand-in op set (tests/fake_ops.py): this file checks the host-side surface, the HIP
kernels are covered by the -m gpu tests.
"""
import ast
import json
import os

import pytest
import torch

from patchfusion_amd.config import make_config
from patchfusion_amd.model import PatchFusion
from patchfusion_amd.registry import MODELS, build_model
from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
from tests.fake_ops import ops as fake_ops

TINY = ("vits", (112, 154), (448, 616), (2, 2))


class ConfigDict(dict):
    """Stand-in with the two properties the reference relies on (patchfusion.py:64-69): the class is called ConfigDict
    (isinstance test) and it offers to_dict() + attribute access.  mmengine itself is not installed in this image."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError as e:
            raise AttributeError(k) from e
        return ConfigDict(v) if isinstance(v, dict) and not isinstance(v, ConfigDict) else v

    def to_dict(self):
        def plain(v):
            if isinstance(v, dict):
                return {k: plain(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return [plain(x) for x in v]
            return v
        return plain(self)


def reference_surface(golden_dir):
    with open(os.path.join(golden_dir, "reference_surface.json")) as f:
        return json.load(f)


def branch_ckpt(sd, prefix, path):
    torch.save({"model_state_dict": {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}}, path)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["vits", "vitb", "vitl"])
def test_shipped_config_files_build_through_the_registry(enc, tmp_path, golden_dir):
    """configs/patchfusion_depthanything/depthanything_{vits,vitb,vitl}_patchfusion_u4k.py:71-90 -> MODELS.build(cfg.model).
    The ConfigDict path forces load_branch=True and loads both branch checkpoints named by `pretrain_model` (strict).
    `model` as running the file yields it (what mmengine.Config.fromfile keeps of it), stored as its repr."""
    model_cfg = ast.literal_eval(reference_surface(golden_dir)["config_model"][enc])
    assert model_cfg["type"] == "PatchFusion" and model_cfg["config"]["coarse_branch"]["midas_model_type"] == enc
    assert MODELS.get("PatchFusion") is PatchFusion
    spec = patchfusion_spec(model_cfg["config"])
    if enc == "vitl":
        # 765 M parameters: check the schema the config yields (keys incl. the 544-channel up-conv) without materialising them twice
        assert spec["guided_fusion.up_conv_list.4.conv.double_conv.0.weight"].shape == (544, 544, 3, 3)
        assert spec["coarse_branch.core.core.pretrained.blocks.23.attn.qkv.weight"].shape == (3072, 1024)
        assert list(model_cfg["config"]["guided_fusion"]["num_patches"]) == [392 * 518, 224 * 296, 112 * 148, 56 * 74, 28 * 37, 14 * 19]
        return
    sd = synthetic_state_dict(spec, 0)
    paths = [str(tmp_path / "coarse.pth"), str(tmp_path / "fine.pth")]
    branch_ckpt(sd, "coarse_branch.", paths[0])
    branch_ckpt(sd, "fine_branch.", paths[1])
    conf = ConfigDict(model_cfg["config"])
    conf["pretrain_model"] = paths
    conf["load_branch"] = False                  # the ConfigDict route must force it to True regardless (patchfusion.py:69)
    m = build_model(dict(type="PatchFusion", config=conf))
    assert isinstance(m, PatchFusion) and m.config.load_branch is True
    got = m.state_dict()
    for k in ("coarse_branch.core.core.pretrained.blocks.0.attn.qkv.weight", "fine_branch.conv2.weight",
              "fine_branch.core.core.depth_head.scratch.refinenet1.resConfUnit1.conv1.weight"):
        assert torch.equal(got[k], sd[k]), k
    assert float(got["guided_fusion.inc.double_conv.0.weight"].abs().max()) == 0.0     # fusion side untouched by the branch ckpts
    assert m.tile_cfg["image_raw_shape"] == (2160, 3840) and m.tile_cfg["patch_raw_shape"] == (540, 960)
    # a wrong branch checkpoint must fail like load_state_dict(strict=True) does
    bad = torch.load(paths[1])
    bad["model_state_dict"].pop("conv2.weight")
    torch.save(bad, paths[1])
    with pytest.raises(RuntimeError, match="Missing key"):
        build_model(dict(type="PatchFusion", config=conf))


def test_vitl_state_dict_keys_match_the_reference_class(golden_dir):
    """state_dict keys / shapes / dtypes of the headline model (DA-vitl) against the reference's own constructor
    (tests/test_spec.py covers vits / vitb)."""
    from oracle.make_golden import schema_digest
    want = reference_surface(golden_dir)["state_dict_sha256"]["vitl"]
    cfg = make_config("vitl", (112, 154), (448, 616), (2, 2))
    spec = patchfusion_spec(cfg)
    assert schema_digest((k, e.shape, e.dtype) for k, e in spec.items()) == want


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    cfg = make_config(*TINY)
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    m = PatchFusion(cfg, compute_dtype="fp32", ops=fake_ops).eval()
    m.load_state_dict(sd, strict=True)
    img = torch.rand(1, 3, *TINY[2], generator=torch.Generator().manual_seed(1234))
    return cfg, sd, m, img


def test_load_dict_and_get_save_dict_like_tools_test_py(tiny):
    """tools/test.py:204-205 prints model.load_dict(ckpt['model_state_dict']); train checkpoints hold get_save_dict()."""
    cfg, sd, m, _ = tiny
    save = m.get_save_dict()
    assert all("coarse_branch" not in k and "fine_branch" not in k for k in save) and len(save) == 456
    m2 = PatchFusion(cfg, compute_dtype="fp32", ops=fake_ops)
    res = m2.load_dict(save)
    assert res.unexpected_keys == [] and all(k.startswith(("coarse_branch.", "fine_branch.")) for k in res.missing_keys)
    assert "missing_keys" in str(res) or "All keys matched" in str(res)
    assert torch.equal(m2.state_dict()["fusion_conv_list.0.weight"], sd["fusion_conv_list.0.weight"])


def test_partial_checkpoint_after_free_parameters_is_refused_and_changes_nothing(tiny):
    """round-5 advisor (medium): after free_parameters() a load_state_dict() that does not cover every tensor (strict=False with the fusion-only
    get_save_dict() format, one branch through _load_branch) used to zero-fill the uncovered tensors, clear the flag and let the next forward rebuild the
    engine from zeros.  Now it raises, the module stays in the released state and the live engine keeps producing the same numbers; a strict load that
    fails (unexpected key) also leaves the released state; a complete dict restores the module."""
    cfg, sd, _, img = tiny
    m = PatchFusion(cfg, compute_dtype="fp32", ops=fake_ops).eval()
    m.load_state_dict(sd, strict=True)
    lr = m.resizer(img)
    with torch.no_grad():
        d0, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=2)
    save = m.get_save_dict()
    m.free_parameters()
    engine = m._engine
    with pytest.raises(RuntimeError, match="must now be given every tensor"):
        m.load_dict(save)                                           # the reference's own strict=False helper with a fusion-only checkpoint
    with pytest.raises(RuntimeError, match="must now be given every tensor"):
        m._load_branch("coarse_branch.", {k[len("coarse_branch."):]: v for k, v in sd.items() if k.startswith("coarse_branch.")})
    assert m._params_freed and m._engine is engine and sum(p.numel() for p in m.parameters()) == 0
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, not_a_key=torch.zeros(1)), strict=True)
    assert m._params_freed and m._engine is engine and sum(p.numel() for p in m.parameters()) == 0
    with torch.no_grad():
        d1, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=2)
    assert torch.equal(d0, d1)
    m.load_state_dict(sd, strict=True)
    assert not m._params_freed and m._engine is None and len(m.state_dict()) == len(sd)
    with torch.no_grad():
        d2, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=2)
    assert torch.equal(d0, d2)


def test_plain_dict_config_never_loads_branch_checkpoints(tiny):
    """HF path (patchfusion.py:70-78): config.json written by tools/convert_huggingface.py carries load_branch=true and
    local ./work_dir paths; a plain-dict config must force load_branch=False instead of torch.load-ing them."""
    cfg, _, _, _ = tiny
    c = dict(cfg, load_branch=True, pretrain_model=["./work_dir/none/coarse.pth", "./work_dir/none/fine.pth"])
    m = PatchFusion(c, ops=fake_ops)
    assert m.config.load_branch is False and m.config.coarse_branch.pretrained_resource is None


def test_hf_save_pretrained_from_pretrained_round_trip(tiny, tmp_path):
    """tools/convert_huggingface.py:78-79: model.save_pretrained(dir); model.config.to_json_file(dir/config.json);
    README: PatchFusion.from_pretrained(...)."""
    cfg, sd, m, img = tiny
    m.config["load_branch"] = True                # what a converted checkpoint's config.json contains
    try:
        m.save_pretrained(str(tmp_path))
        m.config.to_json_file(os.path.join(str(tmp_path), "config.json"))
    finally:
        m.config["load_branch"] = False
    j = json.load(open(tmp_path / "config.json"))
    assert j["load_branch"] is True and j["patch_process_shape"] == [112, 154]
    m2 = PatchFusion.from_pretrained(str(tmp_path), ops=fake_ops)
    assert m2.config.load_branch is False
    a, b = m.state_dict(), m2.state_dict()
    assert list(a.keys()) == list(b.keys()) and all(torch.equal(a[k], b[k]) for k in a)


def test_infer_forward_with_the_reference_call_protocol(tiny):
    """baseline_pretrain.py:275-307 + patchfusion.py:410-414: coarse_forward -> tile_temp -> per batch
    infer_forward(rebatch_image, bbox_feat_forward, tile_temp, coarse_temp_dict).  Must equal forward()'s own tiles, also
    when the coarse tensors handed back are COPIES (foreign tensors -> state rebuilt from tile_temp)."""
    cfg, sd, m, img = tiny
    lr = m.resizer(img)
    with torch.no_grad():
        full, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=2)
        cp, cf = m.coarse_forward(lr)
        tile_cfg = m.tile_cfg
        hr, wr = tile_cfg["patch_raw_shape"]
        crops, boxes = [], []
        for h in tile_cfg["raw_h_split_point"]:
            for w in tile_cfg["raw_w_split_point"]:
                crops.append(m.resizer(img[:, :, h:h + hr, w:w + wr])[0])
                boxes.append([w, h, w + wr, h + hr])
        crops = torch.stack(crops)
        bboxs = torch.tensor(boxes).int()
        H, W = tile_cfg["image_raw_shape"]
        ps = m.patch_process_shape
        fac = torch.tensor([1 / W * ps[1], 1 / H * ps[0], 1 / W * ps[1], 1 / H * ps[0]]).unsqueeze(0)
        bf = torch.cat((torch.arange(4).unsqueeze(-1), bboxs * fac), dim=-1)
        for tile_temp in (dict(coarse_prediction=cp, coarse_features=cf),
                          dict(coarse_prediction=cp.clone(), coarse_features=[f.clone() for f in cf])):
            preds = []
            for i in range(0, 4, 2):
                bb = bf[i:i + 2].clone()
                bb[:, 0] = 0
                preds.append(m.infer_forward(crops[i:i + 2], bb, tile_temp, {"coarse_depth_roi": None, "coarse_feats_roi": None}))
            preds = torch.cat(preds)
            assert preds.shape == (4, 1, *ps)
            # the 2x2 m1 map is the four tiles pasted side by side (blend mask cancels where a single tile covers a pixel)
            tl = full[0, 0, :ps[0], :ps[1]]
            assert float((preds[0, 0] - tl).abs().max()) < 1e-5
            br = full[0, 0, ps[0]:, ps[1]:]
            assert float((preds[3, 0] - br).abs().max()) < 1e-5


def test_tile_temp_reuse_needs_identity_and_unmodified_tensors(tiny):
    """The engine state of the last coarse_forward is reused only for the very tensor OBJECTS it handed out, unmodified: an in-place
    write into them (new coarse data in the same storage) or foreign tensors -- which may sit on recycled addresses -- must rebuild
    the state from tile_temp instead of silently using the stale one (round-2 advisor finding)."""
    cfg, sd, m, img = tiny
    lr = m.resizer(img)
    with torch.no_grad():
        cp, cf = m.coarse_forward(lr)
        st0 = m._coarse_state
        tt = dict(coarse_prediction=cp, coarse_features=cf)
        assert m._state_from_tile_temp(tt) is st0                                  # untouched hand-out -> reuse
        other = m.resizer(torch.rand(1, 3, *img.shape[2:], generator=torch.Generator().manual_seed(77)))
        cp2, cf2 = m.coarse_forward(other)
        want = [f.clone() for f in cf2]
        for a, b in zip(cf, cf2):                                                   # caller refills the FIRST hand-out in place
            a.copy_(b)
        cp.copy_(cp2)
        m._coarse_state = st0                                                       # ... and the engine still holds the old state
        st = m._state_from_tile_temp(tt)
        assert st is not st0
        from patchfusion_amd.model import PatchFusion  # noqa: F401
        nchw = [f.float().permute(0, 3, 1, 2) for f in st["feats"]]
        assert all(float((a - b).abs().max()) < 1e-6 for a, b in zip(nchw, want))  # rebuilt from the NEW data
        # foreign tensors with equal values: rebuilt as well (never matched by address)
        st3 = m._state_from_tile_temp(dict(coarse_prediction=cp.clone(), coarse_features=[f.clone() for f in cf]))
        assert st3 is not st


def test_tile_geometry_equals_the_reference_method_over_many_shapes(golden_dir):
    """tiling.prepare_tile_cfg against the reference's own BaselinePretrain.prepare_tile_cfg (baseline_pretrain.py:91-119), called
    unbound on a stand-in `self`: every key / value for a sweep of raw shapes and splits, and the same AssertionError (message included)
    for shapes that 2 * split does not divide: the sha256 of the reference's answers over the seeded sweep (oracle/make_golden.py tile_sweep),
    which ours must reproduce exactly."""
    from oracle.make_golden import tile_digest, tile_sweep
    from patchfusion_amd import tiling
    answers, n_ok, n_bad = [], 0, 0
    for ps, raw, split in tile_sweep():
        try:
            answers.append(tiling.prepare_tile_cfg(ps, raw, split))
            n_ok += 1
        except AssertionError as e:
            answers.append(str(e))
            n_bad += 1
    assert tile_digest(answers) == reference_surface(golden_dir)["tile_geometry_sha256"]
    assert n_ok > 100 and n_bad > 30, (n_ok, n_bad)
