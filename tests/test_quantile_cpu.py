"""CPU pins of the device quantiles' restatements (tests/_quantile_ref.py): np.percentile / torch.quantile bit for bit, matplotlib's colour rule, the
goldens the reference's colorize() and normalizer wrote, and the new surface (exports, ABI 10, src.util.depth_transform)."""
import ctypes
import glob
import os
import re
import warnings

import numpy as np
import pytest
import torch

import _quantile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_EXPORTS = ("ada_quantile_fwd", "ada_range_map_fwd", "ada_depth_colorize_fwd")
SIZES = (1, 2, 3, 7, 101, 1000, 70001)
PERCENTILES = (0, 2, 5, 33.3, 50, 95, 98, 100)
F32 = np.float32


def _contents(n, seed):
    """name -> fp32 [n]: the value patterns of the issue (NaN-free; the NaN case is its own test)."""
    rng = np.random.default_rng(seed)
    normal = rng.standard_normal(n).astype(F32)
    out = {"normal": normal,
           "eight_values": rng.choice(np.array([-3, -0.5, 0, 0.25, 1, 1.5, 7, 100], F32), n),
           "constant": np.full(n, 2.75, F32),
           "denormals": (rng.integers(-50, 50, n) * np.float64(1.4e-45)).astype(F32),
           "signed_zeros": rng.choice(np.array([-0.0, 0.0, 1e-3, -1e-3], F32), n)}
    inf = normal.copy()
    inf[rng.integers(0, n, max(1, n // 10))] = np.inf
    inf[rng.integers(0, n, max(1, n // 10))] = -np.inf
    out["infinities"] = inf
    return out


def _same_bits(a, b):
    """Bitwise equality, NaN equal to NaN, -0 equal to +0 (equal values: which sign a sort leaves first is unspecified)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype
    if np.isnan(a).any() or np.isnan(b).any():
        return bool(np.array_equal(np.isnan(a), np.isnan(b)))
    if np.all(a == 0) and np.all(b == 0):
        return True
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_numpy_restatement_equals_np_percentile_bitwise(n):
    seen_integer_rank = seen_upper_branch = False
    for name, x in _contents(n, 100 + n).items():
        pops = {"all": x, "masked": R.population(x, valid=np.random.default_rng(n).random(n) < 0.6),
                "positive": R.population(x, positive_only=True), "excluded": R.population(x, exclude_value=x[0])}
        for pname, pop in pops.items():
            if pop.size == 0:
                continue
            for p in PERCENTILES:
                with np.errstate(all="ignore"), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    want = np.percentile(pop.astype(np.float64), p)
                got = R.quantile_numpy(pop, p / 100)
                assert _same_bits(got, np.float64(want)), (name, pname, n, p, got, want)
                v = (pop.size - 1) * (p / 100)
                seen_integer_rank |= v == np.floor(v)
                seen_upper_branch |= (v - np.floor(v)) >= 0.5
    assert seen_integer_rank and (seen_upper_branch or n < 3)


@pytest.mark.parametrize("n", SIZES)
def test_torch_restatement_equals_torch_quantile_bitwise(n):
    for name, x in _contents(n, 200 + n).items():
        pops = {"all": x, "masked": R.population(x, valid=np.random.default_rng(n).random(n) < 0.6), "positive": R.population(x, positive_only=True)}
        for pname, pop in pops.items():
            if pop.size == 0:
                continue
            for q in (0.02, 0.98, 0.1, 0.5, 0.0, 1.0):
                q32 = torch.tensor([q], dtype=torch.float32)
                want = torch.quantile(torch.from_numpy(pop.copy()), q32)[0].numpy()
                got = R.quantile_torch(pop, F32(q))
                assert _same_bits(got, want), (name, pname, n, q, got, want)


def test_an_included_nan_makes_the_result_nan_in_both_references():
    x = np.array([1, 2, np.nan, 4, 5], F32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(np.percentile(x.astype(np.float64), 50)) and np.isnan(R.quantile_numpy(x, 0.5))
    assert torch.isnan(torch.quantile(torch.from_numpy(x), torch.tensor([0.5]))[0]) and np.isnan(R.quantile_torch(x, 0.5))
    # excluded by the population rule it does not count
    assert R.quantile_numpy(R.population(x, positive_only=True), 0.5) == 3.0
    assert R.quantile_torch(R.population(x, valid=~np.isnan(x)), 0.5) == 3.0
    assert np.isnan(R.quantile_numpy(np.zeros(0, F32), 0.5)) and np.isnan(R.quantile_torch(np.zeros(0, F32), 0.5))


def test_fused_multiply_add_restatement_rounds_once():
    rng = np.random.default_rng(5)
    a, b, c = (rng.standard_normal(2000).astype(F32) for _ in range(3))
    exact = a.astype(np.float64) * b.astype(np.float64)      # 48 bits: exact in double
    for i in range(2000):
        got = R.fmaf(a[i], b[i], c[i])
        lo, hi = sorted((np.nextafter(got, F32(-np.inf)), np.nextafter(got, F32(np.inf))))
        t = exact[i] + np.float64(c[i])
        assert np.float64(lo) < t < np.float64(hi)
    assert R.fmaf(F32(np.inf), F32(0), F32(1)) != R.fmaf(F32(np.inf), F32(0), F32(1))      # NaN
    assert R.fmaf(F32(3), F32(0), F32(-0.0)) == 0


@pytest.mark.parametrize("cmap", ["turbo_r", "Spectral_r", "magma_r"])
def test_colour_rule_equals_matplotlib_bytes(cmap):
    import matplotlib
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.random(100000) * 1.4 - 0.2, np.arange(257) / 256.0, np.nextafter(np.arange(257) / 256.0, -1.0),
                        [np.nan, np.inf, -np.inf, 1.0, 0.0, -0.0, 5e-324]])
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = matplotlib.colormaps[cmap](t.copy(), bytes=True)
    idx = R.colour_index(t)
    got = np.where((idx < 0)[:, None], np.zeros(4, np.uint8), R.rgba_lut(cmap)[np.maximum(idx, 0)])
    assert np.array_equal(got, want)


def _golden(kind):
    files = sorted(glob.glob(os.path.join(GOLDEN, kind, "*.npz")))
    assert files, f"no goldens under tests/golden/{kind}"
    return files


@pytest.mark.parametrize("path", _golden("colorize"), ids=os.path.basename)
def test_colorize_restatement_equals_the_references_golden(path):
    g = np.load(path)
    kw = {k[4:]: (g[k] if g[k].ndim and k != "arg_background_color" else (tuple(int(v) for v in g[k]) if g[k].ndim else g[k].item())) for k in g.files if k.startswith("arg_")}
    assert g["value"].dtype == np.float32 and max(g["value"].shape) <= 64
    got = R.colorize(g["value"], **kw)
    assert got.dtype == np.uint8 and np.array_equal(got, g["image"])


@pytest.mark.parametrize("path", _golden("depth_transform"), ids=os.path.basename)
def test_normalizer_restatement_equals_the_references_golden(path):
    g = np.load(path)
    cfg = {k[4:]: g[k].item() for k in g.files if k.startswith("cfg_")}
    valid = g["valid"] if "valid" in g.files else None
    assert max(g["depth"].shape) <= 64
    got = R.normalize(g["depth"], valid, **cfg)
    want = g["out"]
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_golden_tool_is_committed_and_stores_arrays_only():
    src = open(os.path.join(ROOT, "tools", "make_golden_quantile.py")).read()
    assert "ast.parse" in src and "--reference" in src
    for kind in ("colorize", "depth_transform"):
        for path in _golden(kind):
            assert os.path.getsize(path) < 64 * 1024
            with np.load(path, allow_pickle=False) as g:
                assert all(g[k].dtype.kind in "fbiuU" for k in g.files), path


def test_new_exports_and_abi_version():
    import hip_ext
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    assert re.search(r"#define\s+ADA_ABI_VERSION\s+10\b", header) and hip_ext.ABI_VERSION == 10
    lib = hip_ext.load()
    assert lib.ada_abi_version() == 10
    bf16 = ctypes.CDLL(hip_ext.library_path(bf16=True))
    for name in NEW_EXPORTS:
        assert name in hip_ext.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and hasattr(bf16, name), name
    for macro, value in (("ADA_QUANTILE_CHUNK", hip_ext.QUANTILE_CHUNK), ("ADA_QUANTILE_MAX_Q", hip_ext.QUANTILE_MAX_Q),
                         ("ADA_QUANTILE_WS_BYTES_PER_IMAGE", hip_ext.QUANTILE_WS_BYTES_PER_IMAGE), ("ADA_Q_NUMPY", hip_ext.Q_NUMPY),
                         ("ADA_Q_TORCH", hip_ext.Q_TORCH), ("ADA_Q_EXCLUDE_VALUE", hip_ext.Q_EXCLUDE_VALUE), ("ADA_Q_POSITIVE_ONLY", hip_ext.Q_POSITIVE_ONLY)):
        m = re.search(r"#define\s+%s\s+(\S+)" % macro, header)
        assert m and int(m.group(1), 0) == value, macro
    build_py = open(os.path.join(ROOT, "amodal-depth-anything_amd", "csrc", "build.py")).read()
    assert '"ada_quantile.hip"' in re.search(r"^SOURCES\s*=\s*\[([^\]]*)\]", build_py, flags=re.M).group(1)
    assert '"ada_quantile.hip"' in re.search(r"^NO_SCRATCH\s*=\s*\{([^}]*)\}", build_py, flags=re.M).group(1)


def test_host_argument_checks_need_no_device():
    import hip_ext
    from hip_ext import image, quantile
    x = torch.zeros(2, 8)
    for call in (lambda: quantile.quantiles(x, 0.5), lambda: quantile.percentile_range(x), lambda: image.colorize(torch.zeros(1, 4, 4))):
        with pytest.raises(hip_ext.HipExtError):       # no CPU fallback
            call()
    with pytest.raises(ValueError):
        quantile.quantiles(x, 1.5)
    with pytest.raises(ValueError):
        quantile.quantiles(x, 0.5, method="median")
    with pytest.raises(ValueError):
        quantile.percentile_range(x, vminp=-1)
    for kw in ({"gamma_corrected": True}, {"value_transform": lambda v: v}):
        with pytest.raises(NotImplementedError):
            image.colorize(torch.zeros(1, 4, 4), **kw)
    lut = image.colormap_lut_rgba("turbo_r")
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 4) and np.array_equal(lut.numpy(), R.rgba_lut("turbo_r"))
    assert tuple(image.colormap_lut("turbo_r").shape) == (256, 3) and np.array_equal(image.colormap_lut("turbo_r").numpy(), lut.numpy()[:, :3])


def test_depth_transform_surface():
    import types

    import hip_ext
    from src.util import depth_transform as T
    for name in ("get_depth_normalizer", "DepthNormalizerBase", "ScaleShiftDepthNormalizer", "SAMNormalizer"):
        assert hasattr(T, name), name
    ident = T.get_depth_normalizer(None)
    x = torch.arange(4.0)
    assert ident(x) is x
    cfg = types.SimpleNamespace(type="scale_shift_depth", norm_min=-1.0, norm_max=1.0, min_max_quantile=0.02, clip=True)
    n = T.get_depth_normalizer(cfg)
    assert isinstance(n, T.ScaleShiftDepthNormalizer) and isinstance(n, T.DepthNormalizerBase)
    assert n.is_absolute is False and n.far_plane_at_max is True and (n.norm_min, n.norm_max, n.norm_range) == (-1.0, 1.0, 2.0)
    assert n.min_quantile == 0.02 and n.max_quantile == 1.0 - 0.02 and n.clip is True
    assert torch.equal(n.scale_back(torch.tensor([-1.0, 0.0, 1.0])), torch.tensor([0.0, 0.5, 1.0]))
    assert torch.equal(n.denormalize(torch.tensor([1.0])), torch.tensor([1.0]))
    with pytest.raises(hip_ext.HipExtError):           # the transform itself runs on the device only
        n(torch.ones(4, 4))
    s = T.get_depth_normalizer(types.SimpleNamespace(type="sam_depth"))
    assert isinstance(s, T.SAMNormalizer) and s(x) is x and s.denormalize(x) is x
    assert T.DepthNormalizerBase.is_absolute is None and T.DepthNormalizerBase.far_plane_at_max is None
    with pytest.raises(NotImplementedError):
        T.get_depth_normalizer(types.SimpleNamespace(type="other"))
    with pytest.raises(NotImplementedError):
        T.DepthNormalizerBase()


def test_colorize_depth_cli_reads_depth_files_and_parses_its_flags(tmp_path):
    from PIL import Image
    from src.scripts import colorize_depth as C
    from hip_ext import image
    assert C.colorize is image.colorize
    d16 = (np.arange(35, dtype=np.uint16).reshape(5, 7) * 1000)
    Image.fromarray(d16).save(tmp_path / "d.png")
    np.save(tmp_path / "f.npy", d16[None].astype(np.float32) / 7)
    a, b = C.read_depth(str(tmp_path / "d.png")), C.read_depth(str(tmp_path / "f.npy"))
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (5, 7) and np.array_equal(a, d16.astype(np.float32))
    np.save(tmp_path / "bad.npy", np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        C.read_depth(str(tmp_path / "bad.npy"))
    with pytest.raises(SystemExit):
        C.main([str(tmp_path / "d.png")])                       # the output is required
    import hip_ext
    with pytest.raises(hip_ext.HipExtError):                     # no CPU fallback behind the command line either
        C.main([str(tmp_path / "d.png"), str(tmp_path / "o.png"), "--device", "cpu"])


def test_torch_quantile_fuses_the_lerp_product_on_this_host():
    """The device's torch mode rounds lo + w * d once because ATen's CPU lerp is an fmadd.  1200 draws: the fused restatement equals torch.quantile on every
    one, the step-rounded one misses some.  If torch (or a host without FMA) ever rounds twice, THIS test fails -- not a GPU comparison far from the cause."""
    rng = np.random.default_rng(0)
    fused_misses = stepwise_misses = total = 0
    for n in (2, 3, 7, 101, 1000, 70001):
        for _ in range(50):
            x = rng.standard_normal(n).astype(F32)
            for q in (0.02, 0.98, 0.333, 0.5):
                want = torch.quantile(torch.from_numpy(x), torch.tensor([q], dtype=torch.float32))[0].numpy()
                total += 1
                fused_misses += R.quantile_torch(x, F32(q)).tobytes() != want.tobytes()
                stepwise_misses += R.quantile_torch(x, F32(q), fused=False).tobytes() != want.tobytes()
    assert total == 1200 and fused_misses == 0, fused_misses
    assert stepwise_misses > 0, "torch.quantile now rounds the lerp product on its own: ADA_Q_TORCH (csrc/ada_quantile.hip) fuses it"


def test_excluded_value_is_compared_in_double():
    """0.1 is no fp32: a pixel holding fp32(0.1) is not invalid_val=0.1 -- neither for the percentiles nor for the paint (the reference compares the promoted map)."""
    x = np.array([F32(0.1), 1.0, 2.0, 3.0], F32)
    assert R.population(x, exclude_value=0.1).size == 4 and R.population(x, exclude_value=float(F32(0.1))).size == 3
    img = R.colorize(x.reshape(2, 2), invalid_val=0.1)
    assert not (img.reshape(-1, 4) == (128, 128, 128, 255)).all(1).any()
    assert (R.colorize(x.reshape(2, 2), invalid_val=float(F32(0.1))).reshape(-1, 4)[0] == (128, 128, 128, 255)).all()


def test_render_percentiles_needs_device_render(tmp_path):
    import subprocess
    import sys
    from PIL import Image
    sys.path.insert(0, ROOT)
    import infer
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "i.png")
    Image.fromarray(np.zeros((8, 8), np.uint8)).save(tmp_path / "m.png")
    with pytest.raises(ValueError, match="render_percentiles"):
        infer.infer_single_image(str(tmp_path / "i.png"), str(tmp_path / "m.png"), str(tmp_path / "o"), None, None, device="cuda", device_prep=True,
                                 render_percentiles=(2, 95))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--input_image_path", "i", "--input_mask_path", "m", "--output_folder", "o",
                        "--device_prep", "--render_percentiles", "2", "95"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--render_percentiles needs --device_render" in r.stderr
    import inspect
    from hip_ext.pipeline import amodal_infer_image
    assert inspect.signature(amodal_infer_image).parameters["render_percentiles"].default is None
