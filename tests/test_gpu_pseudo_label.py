"""GPU: the pseudo-label chain of the reference's sam_pl_gen_dav2.py on the device (hip_ext/labels.py).

  * ada_label_combine_fwd bit for bit against the numpy restatement (tests/_pil_resample.py combine), which itself reproduces what the real script
    recorded (tests/golden/pseudo_label/, tools/make_pseudo_label_golden.py) bit for bit -- checked here too, on the host;
  * label_from_depths against the recorded reference: masks and everything outside the whole mask exact, scale / shift within rtol 1e-5, atol 1e-6
    (the bound test_gpu_amodal_infer.py uses for the same fit), the label within one code inside the mask on the cases where nothing wraps;
  * pseudo_label_pairs against its own steps called by hand, and a pair alone against the same pair inside a batch: no network tolerance."""
import os

import numpy as np
import pytest
import torch

import _pil_resample as R
from _cases import GOLDEN_DIR, build_product_model, synth_state_dict

pytestmark = pytest.mark.gpu

FIX_DIR = os.path.join(GOLDEN_DIR, "pseudo_label")
FIXTURES = sorted(f[:-4] for f in os.listdir(FIX_DIR) if f.endswith(".npz") and f != "cast_probes.npz")
RAW_CASE = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
S, LABEL = 70, 64


@pytest.fixture(scope="module")
def fixtures():
    return {n: dict(np.load(os.path.join(FIX_DIR, n + ".npz"))) for n in FIXTURES}


def test_the_fixture_set_is_complete(fixtures):
    assert set(FIXTURES) == {"ellipse_partial", "visible_whole", "two_borders", "empty_visible", "overflow"}
    z = fixtures["two_borders"]["ref_whole"]
    assert z[0].any() and z[:, 0].any()
    assert not fixtures["empty_visible"]["ref_visible"].any()
    assert np.array_equal(fixtures["visible_whole"]["ref_visible"], fixtures["visible_whole"]["ref_whole"])


def _combine(hip, whole, occ, mask, ss, label_size, overflow):
    P, h, w = whole.shape
    L = label_size or h
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    label = torch.zeros(P, L, L, dtype=torch.uint16, device="cuda")
    comb = torch.full((P, h, w), -7.0, device="cuda")
    rows = torch.full((P, L), -7, dtype=torch.int32, device="cuda")
    hip.label_combine(dev(whole), dev(occ), dev(mask), dev(ss), label, comb, rows, hip.LABEL_CLIP if overflow == "clip" else hip.LABEL_WRAP)
    torch.cuda.synchronize()
    only = torch.zeros_like(label)                                                   # the optional outputs left out: the same label
    hip.label_combine(dev(whole), dev(occ), dev(mask), dev(ss), only, None, None, hip.LABEL_CLIP if overflow == "clip" else hip.LABEL_WRAP)
    assert torch.equal(only.view(torch.int16), label.view(torch.int16))
    return label.cpu().numpy(), comb.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("overflow", ["wrap", "clip"])
@pytest.mark.parametrize("label_size", [LABEL, None])
def test_combine_is_the_restatement_bit_for_bit(hip, fixtures, label_size, overflow):
    names = FIXTURES + ["nan_pair"]
    zs = [fixtures[n] for n in FIXTURES] + [fixtures["ellipse_partial"]]
    whole = np.stack([z["ref_whole_norm"] for z in zs])
    occ = np.stack([z["ref_occ_norm"] for z in zs])
    mask = np.stack([z["ref_whole"] for z in zs])
    ss = np.stack([z["ref_scale_shift"] for z in zs]).astype(np.float32)
    ss[-1] = np.nan                                                                  # an image whose fit had no support
    label, comb, rows = _combine(hip, whole, occ, mask, ss, label_size, overflow)
    flagged = {}
    for i, name in enumerate(names):
        want_label, want_comb, want_oor = R.combine(whole[i], occ[i], mask[i], ss[i, 0], ss[i, 1], label_size, overflow)
        assert np.array_equal(label[i], want_label), name
        assert np.array_equal(comb[i].view(np.uint32), want_comb.view(np.uint32)), name     # bit pattern: NaN included
        assert int(rows[i].sum()) == want_oor and rows[i].min() >= 0, (name, int(rows[i].sum()), want_oor)
        flagged[name] = want_oor
        if name in FIXTURES and overflow == "wrap" and label_size == LABEL:
            # the restatement on the recorded inputs IS what the reference's own lines 115-117, 121 recorded
            assert np.array_equal(want_comb, fixtures[name]["ref_combined"]) and np.array_equal(want_label, fixtures[name]["ref_label"]), name
    assert flagged["overflow"] > 0 and flagged["nan_pair"] > 0 and flagged["ellipse_partial"] == 0
    if overflow == "wrap":      # the overflow fixture really wraps: a clipped label differs from it
        i = names.index("overflow")
        assert not np.array_equal(label[i], R.combine(whole[i], occ[i], mask[i], ss[i, 0], ss[i, 1], label_size, "clip")[0])


def test_combine_refuses_bad_arguments(hip):
    a = torch.zeros(1, 8, 8, device="cuda")
    m = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    ss = torch.zeros(1, 2, device="cuda")
    out = torch.zeros(1, 4, 4, dtype=torch.uint16, device="cuda")
    lib = hip.load()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.ada_label_combine_fwd(a.data_ptr(), a.data_ptr(), m.data_ptr(), ss.data_ptr(), 1, 8, 8, 4, 4, 0, out.data_ptr(), None, None, stream) == 0
    assert lib.ada_label_combine_fwd(a.data_ptr(), a.data_ptr(), m.data_ptr(), ss.data_ptr(), 1, 8, 8, 4, 4, 2, out.data_ptr(), None, None, stream) == -1
    assert lib.ada_label_combine_fwd(a.data_ptr(), a.data_ptr(), m.data_ptr(), ss.data_ptr(), 1, 8, 8, 4, 4, 0, None, None, None, stream) == -1
    assert lib.ada_label_combine_fwd(a.data_ptr(), a.data_ptr(), m.data_ptr(), ss.data_ptr(), 1, 8, 0, 4, 4, 0, out.data_ptr(), None, None, stream) == -1
    torch.cuda.synchronize()
    with pytest.raises(hip.HipExtError):
        hip.label_combine(a, a, m, ss[:, :1], out)


@pytest.mark.parametrize("name", FIXTURES)
def test_label_from_depths_against_the_recorded_reference(hip, fixtures, name):
    from hip_ext.labels import label_from_depths, pil_resize
    z = fixtures[name]
    visible = pil_resize(z["visible"], (S, S), out="mask", device="cuda")
    whole = pil_resize(z["whole"], (S, S), out="mask", device="cuda")
    assert np.array_equal(visible.cpu().numpy(), z["ref_visible"]) and np.array_equal(whole.cpu().numpy(), z["ref_whole"])
    dev = lambda a: torch.from_numpy(a).cuda()[None]      # noqa: E731
    res = label_from_depths(dev(z["whole_depth"]), dev(z["occ_depth"]), visible[None], whole[None], label_size=LABEL)
    assert res.label.dtype == torch.uint16 and tuple(res.label.shape) == (1, LABEL, LABEL) and tuple(res.combined.shape) == (1, S, S)
    assert res.scale_shift.dtype == torch.float32 and tuple(res.scale_shift.shape) == (1, 2) and tuple(res.out_of_range.shape) == (1,)
    label = res.label[0].cpu().numpy().astype(np.int64)
    ref = z["ref_label"].astype(np.int64)
    inside = R.resize_nearest(z["ref_whole"], (LABEL, LABEL)) > 0
    ss, ref_ss = res.scale_shift[0].cpu().numpy(), z["ref_scale_shift"]
    diff = np.abs(label - ref)
    print(f"{name}: scale, shift = {ss.tolist()} (reference {ref_ss.tolist()}), max |label - ref| inside {int(diff[inside].max())}, outside "
          f"{int(diff[~inside].max())}, out_of_range {int(res.out_of_range[0])}")
    assert np.array_equal(label[~inside], ref[~inside]), "outside the whole mask the label is the occluded map's, exactly"
    assert np.array_equal(res.combined[0].cpu().numpy()[z["ref_whole"] == 0], z["ref_combined"][z["ref_whole"] == 0])
    assert np.allclose(ss, ref_ss, rtol=1e-5, atol=1e-6), (ss, ref_ss)
    if name == "empty_visible":
        assert ss.tolist() == [0.0, 0.0] and ref_ss.tolist() == [0.0, 0.0]
    if name != "overflow":
        assert int(res.out_of_range[0]) == 0
        assert int(diff[inside].max()) <= 1
    else:
        assert int(res.out_of_range[0]) > 0
        clip = label_from_depths(dev(z["whole_depth"]), dev(z["occ_depth"]), visible[None], whole[None], label_size=LABEL, overflow="clip")
        assert torch.equal(clip.combined, res.combined) and not torch.equal(clip.label.view(torch.int16), res.label.view(torch.int16))
        c = clip.combined[0].cpu().numpy()
        t = R.resize_nearest(c, (LABEL, LABEL)) * np.float32(65535.0)
        lab = clip.label[0].cpu().numpy()
        assert (lab[t < 0] == 0).all() and (lab[t >= 65535] == 65535).all()
    # label_size=None: the label at the network size, the same codes before the gather
    full = label_from_depths(dev(z["whole_depth"]), dev(z["occ_depth"]), visible[None], whole[None], label_size=None)
    assert tuple(full.label.shape) == (1, S, S)
    assert np.array_equal(R.resize_nearest(full.label[0].cpu().numpy(), (LABEL, LABEL)), res.label[0].cpu().numpy())


class _Counted(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, []

    def forward(self, x, **kw):
        self.calls.append((tuple(x.shape), dict(kw)))
        return self.inner(x, **kw)


def _photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.4 * np.sin(yy[..., None] * rng.uniform(0.01, 0.2, 3) + xx[..., None] * rng.uniform(0.01, 0.2, 3))
    img = np.clip(base * 255 + rng.normal(0, 30, (h, w, 3)), 0, 255)
    img[h // 3: 2 * h // 3 + 1, w // 4: w // 2 + 1] = (255, 0, 240)
    return np.ascontiguousarray(img.astype(np.uint8))


def _pair(h, w, seed):
    photo = _photo(h, w, seed)
    yy, xx = np.mgrid[0:h, 0:w]
    whole = ((((yy - h * 0.5) / (h * 0.3)) ** 2 + ((xx - w * 0.5) / (w * 0.3)) ** 2) <= 1).astype(np.uint8) * 255
    visible = whole * (xx < w * 0.55).astype(np.uint8)
    occ = photo.copy()
    occ[(whole > 0) & (visible == 0)] = (30, 200, 90)        # the occluder covers the hidden part
    return photo, occ, visible, whole


def test_pseudo_label_pairs_is_its_steps_called_by_hand(hip):
    from hip_ext.labels import label_from_depths, pil_resize, pseudo_label_pairs
    raw = build_product_model(RAW_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    raw = raw.cuda()
    pairs = [_pair(45, 61, 1), _pair(90, 120, 2)]
    cols = [list(c) for c in zip(*pairs)]
    counted = _Counted(raw)
    res = pseudo_label_pairs(counted, *cols, size=S, label_size=LABEL, mask_resample=["bicubic", ("nearest", "bicubic")])
    assert counted.calls == [((4, 3, S, S), dict(normalise_input=True))], counted.calls
    assert tuple(res.label.shape) == (2, LABEL, LABEL) and res.label.is_cuda
    x = torch.stack([pil_resize(img, (S, S), out="float", device="cuda") for img in cols[0] + cols[1]])
    assert tuple(x.shape) == (4, 3, S, S)
    with torch.no_grad():
        depth = raw(x, normalise_input=True).reshape(4, S, S).contiguous()
    vis = torch.stack([pil_resize(cols[2][0], (S, S), out="mask", device="cuda"), pil_resize(cols[2][1], (S, S), "nearest", out="mask", device="cuda")])
    who = torch.stack([pil_resize(m, (S, S), out="mask", device="cuda") for m in cols[3]])
    assert 0 < int(vis[1].sum()) < int(who[1].sum())
    want = label_from_depths(depth[:2], depth[2:], vis, who, label_size=LABEL)
    for got, ref in zip(res, want):
        assert torch.equal(got.view(torch.int16) if got.dtype == torch.uint16 else got, ref.view(torch.int16) if ref.dtype == torch.uint16 else ref)
    assert bool(torch.isfinite(res.scale_shift).all()) and float(res.combined.std()) > 0
    # pair 0 alone = pair 0 inside the batch
    alone = pseudo_label_pairs(raw, *[c[:1] for c in cols], size=S, label_size=LABEL)
    assert torch.equal(alone.label.view(torch.int16), res.label[:1].view(torch.int16))
    assert torch.equal(alone.combined, res.combined[:1]) and torch.equal(alone.scale_shift, res.scale_shift[:1])
    with pytest.raises(ValueError):
        pseudo_label_pairs(raw, cols[0], cols[1][:1], cols[2], cols[3], size=S)


def test_runner_writes_the_labels_of_pseudo_label_pairs(hip, tmp_path):
    """run() over three samples in batches of two: 16-bit PNGs named {id}_depth.png holding pseudo_label_pairs' labels; a 1-bit mask file takes NEAREST."""
    from PIL import Image

    from hip_ext.labels import pseudo_label_pairs
    from src.scripts import sam_pl_gen_dav2 as G
    raw = build_product_model(RAW_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    raw = raw.cuda()
    dirs = {k: tmp_path / k for k in ("image", "occ", "visible", "whole")}
    for d in dirs.values():
        d.mkdir()
    ids = ["7", "12", "305"]
    for i, sid in enumerate(ids):
        photo, occ, visible, whole = _pair(45 + 6 * i, 61 + 4 * i, 10 + i)
        p = G.sample_paths(sid, *(str(dirs[k]) for k in ("image", "occ", "visible", "whole")), str(tmp_path / "out"))
        Image.fromarray(photo).save(p["image"], quality=95)
        Image.fromarray(occ).save(p["occ"])
        (Image.fromarray(visible).convert("1") if i == 1 else Image.fromarray(visible)).save(p["visible"])
        Image.fromarray(whole).save(p["whole"])
    res = G.run(raw, ids, str(dirs["image"]), str(dirs["occ"]), str(dirs["visible"]), str(dirs["whole"]), str(tmp_path / "out"), batch_size=2, size=S,
                label_size=LABEL)
    assert res["samples"] == 3 and res["out_of_range"] >= 0
    for i, sid in enumerate(ids):
        p = G.sample_paths(sid, *(str(dirs[k]) for k in ("image", "occ", "visible", "whole")), str(tmp_path / "out"))
        im = Image.open(p["out"])
        assert im.mode in ("I;16", "I;16B", "I") and im.size == (LABEL, LABEL)
        (vis, vr), (who, wr) = G.load_mask(p["visible"]), G.load_mask(p["whole"])
        assert (vr, wr) == (("nearest" if i == 1 else "bicubic"), "bicubic")
        want = pseudo_label_pairs(raw, [G.load_photo(p["image"])], [G.load_photo(p["occ"])], [vis], [who], size=S, label_size=LABEL, mask_resample=[(vr, wr)])
        assert np.array_equal(np.asarray(im).astype(np.uint16), want.label[0].cpu().numpy())
