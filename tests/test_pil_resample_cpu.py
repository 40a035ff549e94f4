"""CPU: the numpy restatement of Pillow's 8-bit BICUBIC resize, its NEAREST rule and numpy's uint16 cast (tests/_pil_resample.py) against the
installed Pillow called with EXPLICIT filters, byte for byte; hip_ext.labels.pil_coeffs against the restatement's tables; the new C-ABI names; the
pseudo-label runner's chunking, file naming and mode-to-resample choice (no device)."""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image

import _pil_resample as R
from _cases import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ada_hip.h")
FIX_DIR = os.path.join(GOLDEN_DIR, "pseudo_label")
BICUBIC_SHAPES = [((300, 450), (70, 70)), ((40, 30), (70, 70)), ((1500, 2250), (518, 518)), ((97, 70), (70, 70)), ((70, 33), (70, 70)), ((5, 3), (14, 14)),
                  ((2000, 1), (14, 28))]
NEAREST_SHAPES = [((518, 518), (512, 512)), ((56, 56), (99, 99)), ((518, 518), (333, 333)), ((1000, 1000), (7, 7)), ((70, 84), (64, 37)),
                  ((123, 517), (100, 511)), ((517, 123), (333, 99))]


def _pixels(h, w, c, seed):
    """every grey level, hard edges at both ends of the range (the negative lobes overshoot there: the clamp is reached on both sides)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    img[h // 3: h // 2 + 1, w // 4: w // 2 + 1] = (255, 0, 250)[:c]
    img[: max(h // 5, 1), : max(w // 6, 1)] = 0
    return img if c == 3 else np.ascontiguousarray(img[..., 0])


@pytest.mark.parametrize("c", [3, 1], ids=["RGB", "L"])
@pytest.mark.parametrize("hw,out", BICUBIC_SHAPES)
def test_bicubic_restatement_is_pillow_byte_for_byte(hw, out, c):
    img = _pixels(*hw, c, seed=hw[0] + 3 * hw[1])
    want = np.asarray(Image.fromarray(img).resize((out[1], out[0]), Image.BICUBIC))
    got = R.resize_bicubic_u8(img, out)
    assert got.shape == want.shape and int((got != want).sum()) == 0


@pytest.mark.parametrize("hw,out", NEAREST_SHAPES)
def test_nearest_restatement_is_pillow_on_16_bit_images(hw, out):
    a = np.random.default_rng(hw[0]).integers(0, 65536, hw).astype(np.uint16)
    im = Image.fromarray(a)
    assert im.mode == "I;16"
    want = np.asarray(im.resize((out[1], out[0]), Image.NEAREST))
    assert np.array_equal(R.resize_nearest(a, out), want)


def test_pil_coeffs_equal_the_restated_tables():
    from hip_ext.labels import pil_coeffs
    pairs = set()
    for (h, w), (ho, wo) in BICUBIC_SHAPES + NEAREST_SHAPES + [((45, 61), (28, 14)), ((9, 11), (28, 28)), ((64, 1), (14, 28))]:
        pairs |= {(h, ho), (w, wo)}
    for n_in, n_out in sorted(pairs):
        b0, k0, s0 = R.coeffs(n_in, n_out)
        b1, k1, s1 = pil_coeffs(n_in, n_out)
        assert s0 == s1 and b1.dtype == k1.dtype == np.int32 and k1.shape == (n_out, s1), (n_in, n_out)
        assert np.array_equal(b0, b1) and np.array_equal(k0, k1), (n_in, n_out)
    assert pil_coeffs(2250, 518)[2] == 19      # the support grows with the down-scale factor


def test_cast_restatement_equals_the_recorded_numpy_cast():
    z = np.load(os.path.join(FIX_DIR, "cast_probes.npz"))
    got = R.cast_u16(z["values"], "wrap")
    assert np.array_equal(got, z["as_uint16"]), dict(zip(z["values"].tolist(), zip(got.tolist(), z["as_uint16"].tolist())))
    probes = dict(zip(z["values"].tolist(), z["as_uint16"].tolist()))
    f = lambda v: float(np.float32(v))      # noqa: E731
    assert [probes[f(v)] for v in (-3.7, 65536.0, 65537.9, 70000.5, 1e10)] == [65533, 0, 1, 4464, 0]
    assert z["as_uint16"][np.isnan(z["values"])].tolist() == [0]
    clip = R.cast_u16(np.array([-3.7, 65536.0, 70000.5, np.nan, 0.99, 65535.0, 65534.9], np.float32), "clip")
    assert clip.tolist() == [0, 65535, 65535, 0, 0, 65535, 65534]


def test_restatement_reproduces_what_the_reference_script_recorded():
    """masks, paste, cast and the NEAREST label of every fixture, bit for bit, from the recorded normalised maps and the recorded fit"""
    names = sorted(f for f in os.listdir(FIX_DIR) if f.endswith(".npz") and f != "cast_probes.npz")
    assert len(names) == 5
    for f in names:
        z = np.load(os.path.join(FIX_DIR, f))
        assert np.array_equal(R.resize_bicubic_u8(z["visible"], (70, 70)) > 0, z["ref_visible"] > 0), f
        assert np.array_equal(R.resize_bicubic_u8(z["whole"], (70, 70)) > 0, z["ref_whole"] > 0), f
        label, combined, oor = R.combine(z["ref_whole_norm"], z["ref_occ_norm"], z["ref_whole"], *z["ref_scale_shift"], 64, "wrap")
        assert np.array_equal(combined, z["ref_combined"]) and np.array_equal(label, z["ref_label"]), f
        assert (oor > 0) == (f == "overflow.npz"), (f, oor)
        assert z["ref_label"].dtype == np.uint16 and z["ref_label"].shape == (64, 64) and os.path.getsize(os.path.join(FIX_DIR, f)) < 100 * 1024


def test_new_names_are_exported_declared_and_built_under_abi_10():
    import hip_ext
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = hip_ext.load()
    for name in ("ada_pil_resize_u8_fwd", "ada_label_combine_fwd"):
        assert name in hip_ext.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in ada_hip.h"
        assert hasattr(lib, name)
        assert hasattr(ctypes.CDLL(hip_ext.library_path()), name)
    assert hip_ext.ABI_VERSION == 10 and lib.ada_abi_version() == 10
    assert re.search(r"#define\s+ADA_ABI_VERSION\s+10\b", open(HEADER).read())
    assert (hip_ext.PIL_NEAREST, hip_ext.PIL_BICUBIC) == (Image.NEAREST, Image.BICUBIC)


def test_runner_chunks_like_array_split():
    from src.scripts import sam_pl_gen_dav2 as G
    ids = [str(i) for i in range(23)]
    want = np.array_split(ids, int(np.ceil(len(ids) / 5)))           # the script's lines 53-56
    for i, part in enumerate(want):
        assert G.chunk_ids(ids, i, 5) == list(part)
    assert sum(len(G.chunk_ids(ids, i, 5)) for i in range(5)) == 23
    assert G.chunk_ids(ids, 0, 40000) == ids
    with pytest.raises(ValueError):
        G.chunk_ids(ids, 5, 5)
    with pytest.raises(ValueError):
        G.chunk_ids([], 0, 5)


def test_runner_file_names_and_valid_file(tmp_path):
    from src.scripts import sam_pl_gen_dav2 as G
    p = G.sample_paths("1234", "A", "B", "C", "D", "OUT")
    assert p == dict(image=os.path.join("A", "sa_1234.jpg"), occ=os.path.join("B", "1234_occlusion.png"),
                     visible=os.path.join("C", "1234_visible_mask.png"), whole=os.path.join("D", "1234_whole_mask.png"),
                     out=os.path.join("OUT", "1234_depth.png"))
    (tmp_path / "valid.txt").write_text("12\n 7 \n\n9\n")
    assert G.read_valid_file(str(tmp_path / "valid.txt")) == ["12", "7", "9"]


def test_runner_picks_the_resample_pillow_would_and_flattens_colour_masks(tmp_path):
    from src.scripts import sam_pl_gen_dav2 as G
    assert [G.resample_for_mode(m) for m in ("L", "RGB", "1", "P", "RGBA")] == ["bicubic", "bicubic", "nearest", "nearest", "bicubic"]
    m = np.zeros((9, 12), np.uint8)
    m[2:6, 3:9] = 255
    Image.fromarray(m).save(tmp_path / "l.png")
    Image.fromarray(m).convert("1").save(tmp_path / "one.png")
    Image.fromarray(m).convert("P").save(tmp_path / "p.png")
    Image.fromarray(np.stack([m, m, m], -1)).save(tmp_path / "rgb.png")
    for name, mode, resample in (("l", "L", "bicubic"), ("one", "1", "nearest"), ("p", "P", "nearest"), ("rgb", "RGB", "bicubic")):
        assert Image.open(tmp_path / f"{name}.png").mode == mode
        arr, got = G.load_mask(str(tmp_path / f"{name}.png"))
        assert got == resample and arr.dtype == np.uint8 and arr.shape == (9, 12), name
        assert np.array_equal(arr > 0, m > 0), name
    img = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "photo.png")
    assert np.array_equal(G.load_photo(str(tmp_path / "photo.png")), img)
