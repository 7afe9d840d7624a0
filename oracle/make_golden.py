"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/*.npz by running the REFERENCE'S OWN PYTHON
(/root/reference, via oracle/ref_shim.py) on seeded synthetic weights and inputs.

Run in the build container only:   python -m oracle.make_golden
The fixtures travel to the GPU box; the reference does not.

Cases (weights: patchfusion_amd.spec.synthetic_state_dict(seed=0); image: torch.rand with
Generator().manual_seed(1234); python `random` seeded 5621 before every forward, like
tools/test.py:122-123 fix_random_seed):
  tiny_vits : DA-vits, process 112x154, raw 448x616, split 2x2, process_num=2, modes m1 / m2 / r4,
              full output maps + coarse depth + sampled coarse features
  full_vits : DA-vits, process 392x518, raw 784x1036, split 2x2, process_num=4, mode m1, 8192
              sampled output values + stats (kept small)
  cfg4k_vits: BASELINE.json configs[0] and configs[1] themselves - DA-vits, 2160x3840 image:
              2x2 tiles, cai_mode r4, process_num=4 (13 patches; SURVEY 8d "Config 1") and
              4x4 tiles, cai_mode m1, process_num=4 (16 patches; "Config 2"); 16384 sampled values each
              (`python -m oracle.make_golden cfg4k` regenerates only this file; ~5 CPU-minutes)
  variants_vits: the tiny geometry with bin_centers_type / attractor_type / attractor_kind set to the values no shipped config
              uses (patchfusion.py:132-146, attractor.py:112-129), weights seed 3, image seed 11: full m1 map + coarse depth each
              (`python -m oracle.make_golden variants` regenerates only this file)
  headline_vitl_ref: the HEADLINE architecture (DA-vitl, process 392x518) from the reference itself: one 2160x3840 image, 2x2 tiles, m1,
              process_num=4; sampled final map + coarse depth + two coarse feature levels (`python -m oracle.make_golden vitl`; ~1-2 CPU-minutes)
  reference_live.npz + reference_surface.json: what the tests once read from the reference tree at run time (`python -m oracle.make_golden live`):
              the coarse features of the tiny case, BaselinePretrain infer / train outputs, the train-mode forward of PatchFusion (tensors of
              up to 24576 elements whole, larger ones as 8192 seeded samples + whole-tensor stats), the evaluated `model` dict of the shipped
              DA configs, and sha256 digests of the reference class's state-dict schema (vits / vitb / vitl) and of the reference's
              prepare_tile_cfg answers over a seeded sweep of shapes
  cfg2_vitl_ref / cfg3_vitl_ref: the BENCHED configurations themselves from the reference itself - BASELINE.json configs[2] (DA-vitl, 2160x3840,
              4x4 tiles, m1, process_num=8; 16 patches) and the configs[3] geometry (8x8 tiles, m1, process_num=8; 64 patches): the same four
              sampled tensors as headline_vitl_ref (`python -m oracle.make_golden cfg2` ~5 CPU-minutes, `... cfg3` ~20 CPU-minutes on 8 threads)
"""
import hashlib
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from patchfusion_amd.config import make_config  # noqa: E402
from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def sample_idx(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (k,), generator=g).numpy()


def build(enc, ps, raw, split):
    PF = ref_shim.import_reference()
    cfg = make_config(enc, ps, raw, split)
    with ref_shim.in_reference_cwd():
        m = PF(cfg).eval()
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    print(m.load_state_dict(sd, strict=True))
    img = torch.rand(1, 3, *raw, generator=torch.Generator().manual_seed(1234))
    return m, cfg, img


def cfg4k():
    """BASELINE.json configs[0] / configs[1] at their real size, from the reference itself."""
    out = {}
    for name, split, mode in (("c0_2x2_r4", (2, 2), "r4"), ("c1_4x4_m1", (4, 4), "m1")):
        m, cfg, img = build("vits", (392, 518), (2160, 3840), split)
        lr = m.resizer(img)
        with torch.no_grad():
            random.seed(5621)
            d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode=mode, process_num=4)
        flat = d.flatten()
        idx = sample_idx(flat.numel(), 16384, 11)
        out[name + "_shape"] = np.array(d.shape[2:], np.int64)
        out[name + "_idx"] = idx
        out[name + "_val"] = flat[idx].numpy()
        out[name + "_stats"] = np.array([d.mean().item(), d.std().item(), d.min().item(), d.max().item()], np.float32)
        print(name, tuple(d.shape), out[name + "_stats"], flush=True)
        del m
    np.savez_compressed(os.path.join(OUT, "cfg4k_vits.npz"), **out)


def vitl(split=(2, 2), process_num=4, fname="headline_vitl_ref.npz"):
    """(split, process_num, file) = ((2, 2), 4, headline_vitl_ref) | ((4, 4), 8, cfg2_vitl_ref) | ((8, 8), 8, cfg3_vitl_ref).
    The HEADLINE architecture from the reference itself (round-4 review, missing #5): DA-vitl, process 392x518, one 2160x3840 image cut in
    2x2 tiles, cai_mode m1, process_num 4 -- the reference's own PatchFusion.forward(mode='infer') (patchfusion.py:401-453; ViT-L widths
    depth_anything.py:346-352) on the seeded weights / image every headline test uses.  Stored: 8192 sampled values of the final map, 4096 of the
    coarse depth, 2048 of coarse feature level 3 (r2, 256 @ 112x148) and level 5 (out_conv, 32 @ 392x518), + stats.  ~1 CPU-minute on 8 threads."""
    m, cfg, img = build("vitl", (392, 518), (2160, 3840), split)
    lr = m.resizer(img)
    out = {}
    with torch.no_grad():
        random.seed(5621)
        cd, cf = m.coarse_forward(lr)
        d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=process_num)
    for name, t, k, seed in (("depth_m1", d, 8192, 21), ("coarse_depth", cd, 4096, 22), ("coarse_feat3", cf[3], 2048, 23), ("coarse_feat5", cf[5], 2048, 24)):
        flat = t.flatten()
        idx = sample_idx(flat.numel(), k, seed)
        out[name + "_shape"] = np.array(t.shape, np.int64)
        out[name + "_idx"] = idx.astype(np.int32)
        out[name + "_val"] = flat[idx].numpy()
        out[name + "_stats"] = np.array([t.mean().item(), t.std().item(), t.min().item(), t.max().item()], np.float32)
        print(name, tuple(t.shape), out[name + "_stats"], flush=True)
    np.savez_compressed(os.path.join(OUT, fname), **out)


VARIANTS = (("normed", "inv", "mean"), ("hybrid1", "exp", "sum"), ("hybrid2", "inv", "sum"), ("softplus", "exp", "mean"))


def variant_case(kind, atype, akind):
    """config, synthetic weights and image of one variants_vits case (shared with the tests)"""
    cfg = make_config("vits", (112, 154), (448, 616), (2, 2))
    for b in ("coarse_branch", "fine_branch"):
        cfg[b].update(bin_centers_type=kind, attractor_type=atype, attractor_kind=akind)
    sd = synthetic_state_dict(patchfusion_spec(cfg), 3)
    img = torch.rand(1, 3, 448, 616, generator=torch.Generator().manual_seed(11))
    return cfg, sd, img


def variants():
    PF = ref_shim.import_reference()
    out = {}
    for kind, atype, akind in VARIANTS:
        cfg, sd, img = variant_case(kind, atype, akind)
        with ref_shim.in_reference_cwd():
            m = PF(cfg).eval()
        m.load_state_dict(sd, strict=True)
        lr = m.resizer(img)
        with torch.no_grad():
            cd, _ = m.coarse_forward(lr)
            d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=2)
        out[f"{kind}_coarse_depth"] = cd[0, 0].numpy()
        out[f"{kind}_depth_m1"] = d[0, 0].numpy()
        print(kind, atype, akind, float(d.mean()), float(d.std()), float(d.min()), float(d.max()), flush=True)
    np.savez_compressed(os.path.join(OUT, "variants_vits.npz"), **out)


WHOLE_MAX, SAMPLES = 24576, 8192


def tensor_stats(t):
    t = t.double()
    return np.array([t.mean().item(), t.std().item(), t.min().item(), t.max().item()], np.float64)


def put_tensor(out, name, t, seed):
    """one reference tensor of reference_live.npz: whole up to WHOLE_MAX elements, else SAMPLES seeded values + its shape and whole-tensor stats"""
    t = t.detach()
    if t.numel() <= WHOLE_MAX:
        out[name] = t.numpy()
        return
    flat = t.flatten()
    idx = sample_idx(flat.numel(), SAMPLES, seed)
    out[name + "_shape"] = np.array(t.shape, np.int64)
    out[name + "_idx"] = idx.astype(np.int32)
    out[name + "_val"] = flat[idx].numpy()
    out[name + "_stats"] = tensor_stats(t)


def stored_diff(g, name, t):
    """max |t - reference| over what put_tensor kept of the reference tensor: every element, or the samples and the whole-tensor mean / std /
    min / max (none of which moves by more than about the largest elementwise difference).  AssertionError on a shape mismatch."""
    t = t.detach().cpu()
    if name in g.files:
        ref = g[name]
        assert tuple(t.shape) == ref.shape, (name, tuple(t.shape), ref.shape)
        return float(np.abs(t.numpy().astype(np.float64) - ref).max())
    assert tuple(t.shape) == tuple(g[name + "_shape"]), (name, tuple(t.shape), tuple(g[name + "_shape"]))
    v = t.flatten()[torch.from_numpy(g[name + "_idx"].astype(np.int64))].numpy().astype(np.float64)
    return float(max(np.abs(v - g[name + "_val"]).max(), np.abs(tensor_stats(t) - g[name + "_stats"]).max()))


def schema_digest(items):
    """sha256 of a state_dict schema: (key, shape, dtype) in order"""
    rows = [[k, [int(n) for n in shape], str(dtype).replace("torch.", "")] for k, shape, dtype in items]
    return hashlib.sha256(json.dumps(rows).encode()).hexdigest()


def tile_sweep():
    """the 300 seeded (patch_process_shape, raw shape, split) cases of the tile-geometry check, most of them valid"""
    rs = np.random.RandomState(0)
    for _ in range(300):
        split = (int(rs.randint(1, 9)), int(rs.randint(1, 9)))
        ps = (14 * int(rs.randint(2, 30)), 14 * int(rs.randint(2, 40)))
        raw = (int(rs.randint(16, 4400)), int(rs.randint(16, 4400)))
        if rs.rand() < 0.6:
            raw = (raw[0] // (2 * split[0]) * 2 * split[0] or 2 * split[0], raw[1] // (2 * split[1]) * 2 * split[1] or 2 * split[1])
        yield ps, raw, split


def tile_digest(answers):
    """sha256 of prepare_tile_cfg's answers over tile_sweep(): per case its AssertionError message, or every key with its values"""
    rows = [a if isinstance(a, str) else {k: [float(x) for x in np.ravel(v)] for k, v in a.items()} for a in answers]
    return hashlib.sha256(json.dumps(rows, sort_keys=True).encode()).hexdigest()


def live():
    """reference_live.npz + reference_surface.json (see the module docstring); the cases are the ones the tests build themselves."""
    import types
    from collections import OrderedDict

    from patchfusion_amd.config import zoe_branch_config
    from patchfusion_amd.spec import branch_spec
    PF = ref_shim.import_reference()
    from estimator.models.baseline_pretrain import BaselinePretrain as RefBaseline
    out = {}
    # PatchFusion, tiny case: the coarse features (maps and coarse depth are in tiny_vits.npz)
    m, cfg, img = build("vits", (112, 154), (448, 616), (2, 2))
    with torch.no_grad():
        _, cf = m.coarse_forward(m.resizer(img))
    for i, f in enumerate(cf):
        put_tensor(out, f"coarse_feat{i}", f, 300 + i)
    # PatchFusion.forward(mode='train') on tests/test_train_forward_cpu.py's batch
    B, g = 2, torch.Generator().manual_seed(7)
    image_lr = torch.rand(B, 3, 112, 154, generator=g)
    crops = torch.rand(B, 3, 112, 154, generator=g)
    x0 = torch.randint(0, 616 - 308, (B,), generator=g)
    y0 = torch.randint(0, 448 - 224, (B,), generator=g)
    bboxs = torch.stack([x0, y0, x0 + 308, y0 + 224], dim=1)
    gt = 0.3 + torch.rand(B, 1, 112, 154, generator=g)
    gt[:, :, :5] = 0.0
    with torch.no_grad():
        loss, aux = m(mode="train", image_lr=image_lr, image_hr=None, crops_image_hr=crops, crop_depths=gt, bboxs=bboxs)
    out["train_total_loss"] = np.array(float(loss["total_loss"]), np.float64)
    put_tensor(out, "train_depth_pred", aux["depth_pred"], 310)
    del m
    # BaselinePretrain (tests/test_baseline_cpu.py's cases)
    PS, RAW, SPLIT = (112, 154), (448, 616), (2, 2)
    bc = zoe_branch_config("vits", PS)
    for target in ("coarse", "fine"):
        spec = OrderedDict()
        branch_spec(spec, f"{target}_branch.", bc)
        sd = synthetic_state_dict(spec, 0)
        img = torch.rand(1, 3, *RAW, generator=torch.Generator().manual_seed(1234))
        c = ref_shim._AttrDict(bc)
        with ref_shim.in_reference_cwd():
            m = RefBaseline(c, c, dict(type="SILogLoss"), 1e-3, 80, RAW, PS, SPLIT, target=target).eval()
        m.load_dict({k[len(target) + 8:]: v for k, v in sd.items()})
        lr = m.resizer(img)
        for j, mode in enumerate({"coarse": ("m1",), "fine": ("m2", "r1")}[target]):
            with torch.no_grad():
                random.seed(5621)
                d, _ = m(mode="infer", image_lr=lr, image_hr=img, depth_gt=None, cai_mode=mode, process_num=2)
            put_tensor(out, f"baseline_{target}_{mode}", d, 320 + 10 * (target == "fine") + j)
        gg = torch.Generator().manual_seed(77)
        x = torch.rand(2, 3, *PS, generator=gg)
        gt = torch.rand(2, 1, 56, 77, generator=gg) * 3 + 0.2
        gt[0, 0, :5] = 0.0
        with torch.no_grad():
            if target == "coarse":
                loss, aux = m(mode="train", image_lr=x, image_hr=None, depth_gt=gt)
            else:
                loss, aux = m(mode="train", image_lr=x, image_hr=None, depth_gt=None, crops_image_hr=x, crop_depths=gt)
        out[f"baseline_train_{target}_total_loss"] = np.array(float(loss["total_loss"]), np.float64)
        put_tensor(out, f"baseline_train_{target}_depth_pred", aux["depth_pred"], 340 + (target == "fine"))
        del m
    np.savez_compressed(os.path.join(OUT, "reference_live.npz"), **out)
    print("reference_live", {k: v.shape for k, v in out.items()}, flush=True)

    surf = {"config_model": {}, "state_dict_sha256": {}}
    for enc in ("vits", "vitb", "vitl"):
        cfg = make_config(enc, (112, 154), (448, 616), (2, 2))
        with ref_shim.in_reference_cwd():
            ref = PF(cfg)
        surf["state_dict_sha256"][enc] = schema_digest((k, v.shape, v.dtype) for k, v in ref.state_dict().items())
        del ref
        # the evaluated `model` dict of the shipped config file (mmengine's Config.fromfile reduced to running the file)
        path = os.path.join(ref_shim.REF_ROOT, "configs", "patchfusion_depthanything", f"depthanything_{enc}_patchfusion_u4k.py")
        ns = {}
        with open(path) as f:
            exec(compile(f.read(), path, "exec"), ns)
        surf["config_model"][enc] = repr(ns["model"])
    answers = []
    for ps, raw, split in tile_sweep():
        try:
            answers.append(PF.prepare_tile_cfg(types.SimpleNamespace(patch_process_shape=ps), raw, split))
        except AssertionError as e:
            answers.append(str(e))
    surf["tile_geometry_sha256"] = tile_digest(answers)
    with open(os.path.join(OUT, "reference_surface.json"), "w") as f:
        json.dump(surf, f, indent=1)
    print("reference_surface", surf["state_dict_sha256"], surf["tile_geometry_sha256"], flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(os.cpu_count())
    if len(sys.argv) > 1 and sys.argv[1] == "cfg4k":
        cfg4k()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "variants":
        variants()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "live":
        live()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "vitl":
        vitl()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "cfg2":
        vitl((4, 4), 8, "cfg2_vitl_ref.npz")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "cfg3":
        vitl((8, 8), 8, "cfg3_vitl_ref.npz")
        return
    # ---------------- tiny ----------------
    m, cfg, img = build("vits", (112, 154), (448, 616), (2, 2))
    lr = m.resizer(img)
    out = {}
    with torch.no_grad():
        cd, cf = m.coarse_forward(lr)
        out["coarse_depth"] = cd.numpy()
        for i, f in enumerate(cf):
            flat = f.flatten()
            idx = sample_idx(flat.numel(), 2048, 100 + i)
            out[f"coarse_feat{i}_idx"] = idx
            out[f"coarse_feat{i}_val"] = flat[idx].numpy()
            out[f"coarse_feat{i}_stats"] = np.array([f.mean().item(), f.std().item(), f.abs().max().item()], np.float32)
        for mode in ("m1", "m2", "r4"):
            random.seed(5621)
            d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode=mode, process_num=2)
            out[f"depth_{mode}"] = d[0, 0].numpy()
    np.savez_compressed(os.path.join(OUT, "tiny_vits.npz"), **out)
    print("tiny_vits done", {k: v.shape for k, v in out.items() if k.startswith("depth")})
    # ---------------- full-size vits ----------------
    m, cfg, img = build("vits", (392, 518), (784, 1036), (2, 2))
    lr = m.resizer(img)
    out = {}
    with torch.no_grad():
        random.seed(5621)
        cd, cf = m.coarse_forward(lr)
        d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=4)
    for name, t in (("coarse_depth", cd), ("depth_m1", d)):
        flat = t.flatten()
        idx = sample_idx(flat.numel(), 8192, 7)
        out[name + "_idx"] = idx
        out[name + "_val"] = flat[idx].numpy()
        out[name + "_stats"] = np.array([t.mean().item(), t.std().item(), t.min().item(), t.max().item()], np.float32)
    np.savez_compressed(os.path.join(OUT, "full_vits.npz"), **out)
    print("full_vits done", out["depth_m1_stats"])
    cfg4k()
    variants()
    live()
    vitl()
    vitl((4, 4), 8, "cfg2_vitl_ref.npz")
    vitl((8, 8), 8, "cfg3_vitl_ref.npz")


if __name__ == "__main__":
    main()
