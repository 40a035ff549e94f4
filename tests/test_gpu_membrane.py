"""GPU: the membrane solve on the device (csrc/ada_membrane.hip, hip_ext.inpaint.fill_harmonic / blend_seamless) against the numpy / scipy restatement
of its contract (tests/_membrane_ref.py), and what is built on it: amodal_infer_image(blend="seamless"), fill_view / remove_objects and
``depth_to_view --fill_holes harmonic``.

ACCURACY.  Nothing of a conjugate-gradient solve is compared bit for bit with numpy.  With u_ref the direct solve, r(.) the max-norm residual that THIS
file evaluates in numpy fp64 from the fp64 solution the device returns, and kappa = max(A^-1 1) = the infinity norm of A^-1 (A is an M-matrix):
    max |u_dev - u_ref| <= kappa (r(u_dev) + r(u_ref) + 32 * 2^-53 max |x|),
the last term being the rounding of evaluating one residual row (four differences of magnitude <= 2 max |x| and their sum).  Convergence is asserted at
tol = 1e-9 within twice the steps the reference's own conjugate gradients take from zero.  Where the contract promises bits -- untouched pixels, repeated
calls, batches, split iteration counts, workspace contents -- the comparison is np.array_equal on integer views.

Shapes sit one under, on and one over the tile of a workgroup (MEMBRANE_TILE_H x MEMBRANE_TILE_W, also the partition of every reduction) and over twice
it, so the number of partial sums crosses 1 -> 2 -> several.  Masks differ per image of a batch.  Values are quarter-integers in a range of nine; NaN and
+-inf are planted only under pixels that are not known, where they must change nothing.  Workspaces are pre-filled with 0xFF bytes."""
import functools

import numpy as np
import pytest
import torch

import _membrane_ref as R
import hip_ext as HIP

pytestmark = pytest.mark.gpu

F = np.float32
TH, TW = HIP.MEMBRANE_TILE_H, HIP.MEMBRANE_TILE_W
TOL = 1e-9
EPS_ROW = 32 * 2.0 ** -53      # times max |x|: the rounding of one evaluated residual row
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 3), (1, 5, 5), (2, 33, 65), (3, 9, 70),
          (1, TH - 1, TW - 1), (1, TH, TW), (1, TH + 1, TW + 1), (1, 2 * TH + 1, 2 * TW + 3)]
KINDS = ["random5", "random60", "single", "none", "all", "checker", "ring", "disc", "pair", "l_domain", "two_parts"]


def one_case(kind, h, w, seed):
    """(known uint8 [h, w], domain uint8 [h, w] or None)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind in ("random5", "random60"):
        return (rng.random((h, w)) < (0.05 if kind == "random5" else 0.6)).astype(np.uint8) * 3, None      # any non-zero value counts
    if kind == "single":
        v = np.zeros((h, w), np.uint8)
        v[rng.integers(h), rng.integers(w)] = 255
        return v, None
    if kind == "none":
        return np.zeros((h, w), np.uint8), None
    if kind == "all":
        return np.ones((h, w), np.uint8), None
    if kind == "checker":
        return ((yy + xx + seed) % 2).astype(np.uint8), None
    if kind == "ring":
        return ((yy == 0) | (yy == h - 1) | (xx == 0) | (xx == w - 1)).astype(np.uint8), None
    if kind == "disc":
        r = max(min(h, w) / 3.0, 0.75)
        return (((yy - (h - 1) / 2.0) ** 2 + (xx - (w - 1) / 2.0) ** 2) > r * r).astype(np.uint8), None
    if kind == "pair":
        v = np.zeros((h, w), np.uint8)
        r, c = h // 4, w // 5
        v[r, c] = v[h - 1 - r, w - 1 - c] = 1
        return v, None
    if kind == "l_domain":      # an L whose known pixels all lie in the upright arm; known pixels outside the L count for nothing
        d = ((xx < max(w // 3, 1)) | (yy >= h - max(h // 3, 1))).astype(np.uint8) * 5
        v = ((rng.random((h, w)) < 0.3) & (yy < h - max(h // 3, 1))).astype(np.uint8)
        v[0, 0] = 1
        return v, d
    assert kind == "two_parts"      # two components of the domain, a known pixel in the left one only
    d = np.ones((h, w), np.uint8)
    d[:, w // 2] = 0
    v = np.zeros((h, w), np.uint8)
    v[h // 2, 0] = 1
    v[0, w // 2] = 1      # on the gap: outside the domain
    return v, d


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(known [B, h, w], domain [B, h, w] (all ones where a kind has none), x fp32 [B, 3, h, w] with NaN / inf under pixels that are not known, clean x):
    image b takes the kind b places on in KINDS."""
    B, h, w = shape
    k0 = KINDS.index(kind)
    seed = (B * 131 + h) * 1031 + w + k0
    pairs = [one_case(KINDS[(k0 + b) % len(KINDS)], h, w, seed + b) for b in range(B)]
    known = np.stack([p[0] for p in pairs])
    domain = np.stack([np.ones((h, w), np.uint8) if p[1] is None else p[1] for p in pairs])
    rng = np.random.default_rng(seed)
    clean = (rng.integers(0, 9, (B, 3, h, w)) / 4.0 - 1.0).astype(F)
    clean[:, :, 0, 0] = -0.0      # compared as bits wherever (0, 0) keeps its value
    x = clean.copy()
    for b in range(B):
        free = np.flatnonzero(((known[b] != 0) & (domain[b] != 0)).reshape(-1) == 0)
        for c in range(3):
            for p, bad in zip(rng.permutation(free)[:3], (np.nan, np.inf, -np.inf)):
                x[b, c].reshape(-1)[p] = bad
    for a in (known, domain, x, clean):
        a.setflags(write=False)
    return known, domain, x, clean


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """Per plane (b, c): dict(A, b, unk, u, kappa, steps, res) -- the direct solve, the norm of the inverse, the steps of the reference's conjugate
    gradients from zero at TOL and the direct solve's own residual; and per image the unreached pixels."""
    known, domain, x, _ = case(shape, kind)
    planes, un = {}, []
    for b in range(shape[0]):
        k, d = R.masks(known[b], domain[b], shape[1:])
        un.append(R.unreached(k, d) & ~k)
        for c in range(3):
            A, rhs, unk = R.system(x[b, c], known[b], domain[b])
            u = R.solve_direct(A, rhs)
            steps = R.cg(A, rhs, np.zeros(rhs.size), TOL, 100000)[1]
            planes[b, c] = dict(A=A, b=rhs, unk=unk, u=u, kappa=R.kappa(A), steps=steps, res=R.residual(A, rhs, u))
    return planes, np.stack(un)


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()      # a copy: the cached cases are read-only


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.int64)


def workspace(hip, shape4, fill=0xFF):
    B, C, h, w = shape4
    return torch.full((hip.membrane_workspace_bytes(B, C, h, w),), fill, dtype=torch.uint8, device="cuda")


def solve(hip, x, known, domain, counts, guess=None, minus=None, ws=None, tol=TOL):
    """begin -> iterate(n) for n in counts -> end on the device.  Returns host arrays (out fp32, out64, residual, iterations, converged) per plane [B, C]."""
    dx = x if isinstance(x, torch.Tensor) else dev(x)
    B, C, h, w = dx.shape
    ws = workspace(hip, dx.shape) if ws is None else ws
    dk, dd = dev((known != 0).astype(np.uint8)), None if domain is None else dev((domain != 0).astype(np.uint8))
    dm = None if minus is None else dev(minus)
    hip.membrane_begin(dx, dk, ws, domain=dd, guess=None if guess is None else dev(guess), minus=dm, tol=tol)
    for n in counts:
        hip.membrane_iterate(dx, ws, n)
    out = torch.full(dx.shape, float("nan"), dtype=torch.float32, device="cuda")
    out64 = torch.full(dx.shape, float("nan"), dtype=torch.float64, device="cuda")
    res = torch.full((B * C,), -1.0, dtype=torch.float64, device="cuda")
    it = torch.full((B * C,), -1, dtype=torch.int32, device="cuda")
    cv = torch.full((B * C,), 9, dtype=torch.uint8, device="cuda")
    hip.membrane_end(dx, ws, res, it, cv, out=out, out64=out64, plus=dm)
    torch.cuda.synchronize()
    return host(out), host(out64), host(res).reshape(B, C), host(it).reshape(B, C), host(cv).reshape(B, C)


def reached_domain(shape, kind):
    """The domain the Python layer hands to the kernels: the reached part (an unreached component is a singular block and stays out of the solve)."""
    known, domain, _, _ = case(shape, kind)
    un = reference(shape, kind)[1]
    return ((domain != 0) & ~un).astype(np.uint8)


def check_planes(planes, x, out, out64, res, it, cv, cap, what):
    """The accuracy, convergence and report assertions for every plane of a run."""
    for (b, c), p in planes.items():
        if c >= x.shape[1]:
            continue
        xmax = float(np.max(np.abs(p["known_vals"]))) if p["known_vals"].size else 0.0
        u = out64[b, c][p["unk"]]
        r_dev = R.residual(p["A"], p["b"], u)
        err = float(np.max(np.abs(u - p["u"]))) if u.size else 0.0
        bound = p["kappa"] * (r_dev + p["res"] + EPS_ROW * xmax)
        print(f"{what} plane {(b, c)}: unknowns {u.size} kappa {p['kappa']:.3g} steps dev {it[b, c]} ref {p['steps']} cap {cap} r_dev {r_dev:.3g} reported {res[b, c]:.3g} "
              f"err {err:.3g} bound {bound:.3g}")
        assert cv[b, c] == 1, f"{what} plane {(b, c)}: not converged after {it[b, c]} steps, residual {res[b, c]}"
        assert 0 <= it[b, c] <= cap
        assert abs(res[b, c] - r_dev) <= EPS_ROW * xmax and res[b, c] <= TOL
        assert err <= bound, f"{what} plane {(b, c)}: error {err} above the bound {bound}"


def with_known_values(shape, kind, x=None):
    """reference()'s planes with the known values of each plane attached (max |x| of the bound is taken over them)."""
    known, domain, xc, _ = case(shape, kind)
    x = xc if x is None else x
    planes = reference(shape, kind)[0]
    out = {}
    for (b, c), p in planes.items():
        k = (known[b] != 0) & (domain[b] != 0)
        out[b, c] = dict(p, known_vals=x[b, c][k])
    return out


CASES = [(s, k) for s in SHAPES for k in KINDS[:9]] + [(s, k) for s in [(1, 5, 5), (2, 33, 65), (1, TH + 1, TW + 1), (1, 2 * TH + 1, 2 * TW + 3)] for k in KINDS[9:]]


def test_the_shapes_cross_the_tile_counts():
    tiles = sorted({-(-h // TH) * -(-w // TW) for _, h, w in SHAPES})
    assert tiles[0] == 1 and 2 in tiles and max(tiles) >= 6 and max(h * w for _, h, w in SHAPES) <= 70 * 300


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_solve_meets_the_error_bound_and_keeps_the_promised_bits(hip, shape, kind):
    from hip_ext import inpaint
    known, domain, x, clean = case(shape, kind)
    planes, un = with_known_values(shape, kind), reference(shape, kind)[1]
    cap = 2 * max(p["steps"] for p in planes.values())
    dom = reached_domain(shape, kind)
    out, out64, res, it, cv = solve(hip, x, known, dom, [cap])      # C = 3, zero start
    check_planes(planes, x, out, out64, res, it, cv, cap, f"{shape} {kind}")
    if all(kk in ("none", "all") for kk in [KINDS[(KINDS.index(kind) + b) % len(KINDS)] for b in range(shape[0])]):
        assert (it == 0).all()
    for b in range(shape[0]):
        if KINDS[(KINDS.index(kind) + b) % len(KINDS)] in ("none", "all"):
            assert (it[b] == 0).all()
    unknown = np.stack([[planes[b, c]["unk"] for c in range(3)] for b in range(shape[0])])
    assert np.array_equal(bits(out)[unknown], bits(out64.astype(F))[unknown])      # one rounding, of the very fp64 value
    assert np.array_equal(bits(out)[~unknown], bits(x)[~unknown])                  # known, unreached (outside the reached domain) and outside: x's bits
    assert np.array_equal(bits64(out64)[~unknown], bits64(x.astype(np.float64))[~unknown])
    # C = 1: a plane alone gives the bytes it gives among three
    one = solve(hip, x[:, 1:2], known, dom, [cap])
    assert np.array_equal(bits64(one[1][:, 0]), bits64(out64[:, 1])) and np.array_equal(one[3][:, 0], it[:, 1]) and np.array_equal(bits64(one[2][:, 0]), bits64(res[:, 1]))
    # the public call: the same bytes on the solved pixels, ``empty`` on the unreached ones, x's bits elsewhere
    got, (r2, i2, c2) = inpaint.fill_harmonic(dev(x), dev(known), domain=dev(domain), empty=-2.5, guess="zero", max_iter=max(cap, 1), return_info=True)
    want = out.copy()
    want[np.broadcast_to(un[:, None], want.shape)] = -2.5
    assert got.dtype == torch.float32 and np.array_equal(bits(host(got)), bits(want))
    assert np.array_equal(host(i2), it) and np.array_equal(host(c2), cv) and np.array_equal(bits64(host(r2)), bits64(res))
    keep = np.broadcast_to(((known != 0) & (domain != 0))[:, None] | (domain == 0)[:, None], x.shape)
    assert np.array_equal(bits(host(got))[keep], bits(x)[keep])      # -0.0 stays -0.0, the planted NaN / inf outside the domain stay what they were


@pytest.mark.parametrize("shape,kind", [((2, 33, 65), "random5"), ((1, 2 * TH + 1, 2 * TW + 3), "disc"), ((3, 9, 70), "single"), ((2, 33, 65), "l_domain")],
                         ids=lambda v: str(v).replace(" ", ""))
def test_smooth_guess_meets_the_same_bound_within_the_same_cap(hip, shape, kind):
    from hip_ext import inpaint
    known, domain, x, clean = case(shape, kind)
    planes = with_known_values(shape, kind)
    cap = 2 * max(p["steps"] for p in planes.values())
    dom = reached_domain(shape, kind)
    k = ((known != 0) & (domain != 0)).astype(np.uint8)
    guess = host(inpaint.fill_smooth(dev(x), dev(k), empty=0.0))
    out, out64, res, it, cv = solve(hip, x, known, dom, [cap], guess=guess)
    check_planes(planes, x, out, out64, res, it, cv, cap, f"{shape} {kind} smooth")
    got = inpaint.fill_harmonic(dev(x), dev(known), domain=dev(domain), empty=0.0, max_iter=max(cap, 1))      # guess="smooth" is the default
    un = reference(shape, kind)[1]
    want = out.copy()
    want[np.broadcast_to(un[:, None], want.shape)] = 0.0
    assert np.array_equal(bits(host(got)), bits(want))


EXACT = [((2, 33, 65), "random5"), ((1, 2 * TH + 1, 2 * TW + 3), "disc")]


@pytest.mark.parametrize("shape,kind", EXACT, ids=lambda v: str(v).replace(" ", ""))
def test_same_bytes_twice_alone_in_a_batch_and_with_split_counts(hip, shape, kind):
    known, domain, x, _ = case(shape, kind)
    planes = reference(shape, kind)[0]
    n = max(p["steps"] for p in planes.values()) // 2 + 3      # mid-solve: the slow planes are still moving, so an order that differed would show
    dom = reached_domain(shape, kind)
    first = solve(hip, x, known, dom, [n])
    again = solve(hip, x, known, dom, [n])
    split = solve(hip, x, known, dom, [n // 3, 0, n - n // 3 - n // 4, n // 4])
    other = solve(hip, x, known, dom, [n], ws=workspace(hip, x.shape, fill=0x00))
    used = workspace(hip, x.shape)
    solve(hip, np.full(x.shape, 1e30, F), np.ones_like(known), None, [3], ws=used)      # a busier call left its state behind
    reused = solve(hip, x, known, dom, [n], ws=used)
    for what, run in (("twice", again), ("split counts", split), ("workspace 0x00", other), ("used workspace", reused)):
        assert np.array_equal(bits64(run[1]), bits64(first[1])) and np.array_equal(bits(run[0]), bits(first[0])), what
        assert np.array_equal(bits64(run[2]), bits64(first[2])) and np.array_equal(run[3], first[3]) and np.array_equal(run[4], first[4]), what
    assert (first[3] == n).any() and (first[4] == 0).any() and (first[3] <= n).all()      # somebody was not done yet
    for b in range(shape[0]):
        alone = solve(hip, x[b:b + 1], known[b:b + 1], dom[b:b + 1], [n])
        assert np.array_equal(bits64(alone[1][0]), bits64(first[1][b])) and np.array_equal(bits64(alone[2][0]), bits64(first[2][b])), f"image {b} alone"


def test_check_every_stops_early_with_the_same_bytes(hip):
    from hip_ext import inpaint
    shape, kind = (2, 33, 65), "random5"
    known, domain, x, _ = case(shape, kind)
    a, ia = inpaint.fill_harmonic(dev(x), dev(known), empty=-2.5, return_info=True)      # the default cap, every launch issued
    b, ib = inpaint.fill_harmonic(dev(x), dev(known), empty=-2.5, check_every=8, return_info=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for s, t in zip(ia, ib):
        assert torch.equal(s, t)
    assert bool(ia[2].all()) and int(ia[1].max()) < inpaint.default_max_iter(33, 65) // 4


def guarded(need, fill):
    G = 4096
    buf = torch.full((G + need + G,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = buf[G:G + need]
    ws.fill_(fill)

    def check(what):
        torch.cuda.synchronize()
        assert bool((buf[:G] == 0x5A).all()) and bool((buf[G + need:] == 0x5A).all()), f"{what}: guard bytes around the {need}-byte workspace overwritten"
    return ws, check


@pytest.mark.parametrize("shape", [(2, 33, 65), (1, 1, 1), (1, TH + 1, TW + 1)], ids=str)
def test_workspace_size_and_guards(hip, shape):
    B, h, w = shape
    known, domain, x, _ = case(shape, "random5")
    for C in (1, 3):
        tiles = -(-h // TH) * -(-w // TW)
        need = hip.membrane_workspace_bytes(B, C, h, w)
        assert need == -(-(40 * B * C * h * w + 24 * B * C * tiles + 48 * B * C + B * h * w) // 8) * 8
        ws, check = guarded(need, 0xFF)
        solve(hip, x[:, :C], known, None, [4], ws=ws)
        check(f"membrane {shape} C={C}")
        short, check = guarded(need - 8, 0x00)
        dx, dk = dev(x[:, :C]), dev(known)
        with pytest.raises(hip.HipExtError, match="workspace"):
            hip.membrane_begin(dx, dk, short)
        with pytest.raises(hip.HipExtError, match="workspace"):
            hip.membrane_iterate(dx, short, 1)
        check("the refused calls")
    with pytest.raises(hip.HipExtError, match="tol"):
        hip.membrane_begin(dev(x), dev(known), workspace(hip, x.shape), tol=float("nan"))
    with pytest.raises(hip.HipExtError, match="iterations"):
        hip.membrane_iterate(dev(x), workspace(hip, x.shape), -1)


def test_a_slow_image_does_not_disturb_a_finished_one(hip):
    """A batch whose first image (one known pixel) needs about ten times the steps of its second (60 % known): the second freezes early and idles."""
    h, w = 33, 65
    rng = np.random.default_rng(3365)
    known = np.stack([one_case("single", h, w, 1)[0], one_case("random60", h, w, 2)[0]])
    x = (rng.integers(0, 9, (2, 1, h, w)) / 4.0 - 1.0).astype(F)
    steps = []
    for b in range(2):
        A, rhs, _ = R.system(x[b, 0], known[b])
        steps.append(R.cg(A, rhs, np.zeros(rhs.size), TOL, 100000)[1])
    assert steps[0] >= 8 * steps[1]
    cap = 2 * max(steps)
    out, out64, res, it, cv = solve(hip, x, known, None, [cap])
    assert (cv == 1).all() and it[0, 0] >= 5 * it[1, 0] and it[1, 0] <= 2 * steps[1]
    for b in range(2):
        alone = solve(hip, x[b:b + 1], known[b:b + 1], None, [cap])
        assert np.array_equal(bits64(alone[1][0]), bits64(out64[b])) and alone[3][0, 0] == it[b, 0]


def test_a_nan_in_a_known_pixel_costs_only_its_plane(hip):
    """The freeze rule: the plane whose data is not a number reports converged = 0; the other planes' bytes are what they are without it."""
    shape, kind = (2, 33, 65), "random5"
    known, domain, x, _ = case(shape, kind)
    planes = reference(shape, kind)[0]
    cap = 2 * max(p["steps"] for p in planes.values())
    clean_run = solve(hip, x, known, None, [cap])
    bad = np.array(x, copy=True)
    unk = np.pad(known[1] == 0, 1)
    beside = unk[:-2, 1:-1] | unk[2:, 1:-1] | unk[1:-1, :-2] | unk[1:-1, 2:]
    r, c = np.argwhere((known[1] != 0) & beside)[3]      # a known pixel with an unknown neighbour: its value enters the system
    bad[1, 2, r, c] = np.nan
    out, out64, res, it, cv = solve(hip, bad, known, None, [cap])
    assert cv[1, 2] == 0 and it[1, 2] == 0 and np.isnan(res[1, 2])
    others = np.ones((2, 3), bool)
    others[1, 2] = False
    assert (cv[others] == 1).all()
    assert np.array_equal(bits64(out64[others]), bits64(clean_run[1][others])) and np.array_equal(it[others], clean_run[3][others])


def test_input_forms_and_uint8(hip):
    from hip_ext import inpaint
    shape, kind = (2, 33, 65), "random60"
    known, domain, x, clean = case(shape, kind)
    planes, un = reference(shape, kind)
    full = np.stack([[R.fill(x[b, c], known[b], domain[b], empty=-2.5) for c in range(3)] for b in range(2)])
    got = host(inpaint.fill_harmonic(x[0, 0], known[0], domain=domain[0], empty=-2.5))      # numpy [h, w] in, [h, w] out
    assert got.shape == shape[1:] and np.abs(got - full[0, 0]).max() <= 1e-6
    got = host(inpaint.fill_harmonic(dev(x[:, 1]), dev(known).bool(), domain=dev(domain).bool(), empty=-2.5, check_every=16))      # [B, h, w], bool masks
    assert got.shape == shape and np.abs(got - full[:, 1]).max() <= 1e-6
    u8 = np.random.default_rng(7).integers(0, 256, (2, 33, 65, 3), dtype=np.uint8)      # an image: filled as fp32 planes, rounded half to even
    got8 = host(inpaint.fill_harmonic(dev(u8), dev(known), empty=9.0))
    want8 = np.stack([np.stack([R.fill(u8[b, :, :, c], known[b], None, empty=9.0) for c in range(3)], axis=-1) for b in range(2)])
    assert got8.dtype == np.uint8 and got8.shape == u8.shape
    off = np.abs(got8.astype(np.float64) - want8)
    assert off.max() <= 0.5 + 1e-4 and np.array_equal(got8[known != 0], u8[known != 0])
    with pytest.raises(hip.HipExtError, match="HIP device"):
        inpaint.fill_harmonic(torch.from_numpy(clean.copy()), dev(known))


def test_fill_harmonic_inside_a_stream_capture(hip):
    from hip_ext import inpaint
    shape = (2, 33, 65)
    known, domain, x, _ = case(shape, "random5")
    dk, dx = dev(known), dev(x)
    want = inpaint.fill_harmonic(dx, dk, empty=-2.5, max_iter=300)
    run = lambda: inpaint.fill_harmonic(dx, dk, empty=-2.5, max_iter=300)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    dk.copy_(dev(case(shape, "disc")[0]))
    graph.replay()
    torch.cuda.synchronize()
    dk.copy_(dev(known))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- what is built on the solve ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("partial", [False, True], ids=["perez", "partial-known"])
def test_blend_seamless_against_the_restatement(hip, partial):
    from hip_ext import inpaint
    B, h, w = 2, 33, 65
    rng = np.random.default_rng(3365 + partial)
    src = (rng.integers(0, 9, (B, 1, h, w)) / 4.0 - 1.0).astype(F)
    dst = (rng.integers(0, 9, (B, 1, h, w)) / 4.0 + 2.0).astype(F)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = np.stack([(((yy - 16) / 11.0) ** 2 + ((xx - 30) / 22.0) ** 2 <= 1), (yy > 8) & (yy < 30) & (xx > 40)]).astype(np.uint8)
    known = None
    if partial:      # only the part of the outside above the object pins the correction, and a few pixels inside it
        known = ((mask == 0) & (yy[None] < 14)).astype(np.uint8)
        known[:, 16, 30] = 1
    k = (mask == 0) if known is None else (known != 0)
    d = (mask != 0) | k
    diff = np.where(k[:, None], dst.astype(np.float64) - src.astype(np.float64), 0.0)      # exact: both are quarter-integers
    assert np.array_equal(diff.astype(F).astype(np.float64), diff)
    planes, steps = {}, []
    for b in range(B):
        A, rhs, unk = R.system(diff[b, 0], k[b], d[b])
        u = R.solve_direct(A, rhs)
        steps.append(R.cg(A, rhs, np.zeros(rhs.size), TOL, 100000)[1])
        planes[b, 0] = dict(A=A, b=rhs, unk=unk, u=u, kappa=R.kappa(A), steps=steps[-1], res=R.residual(A, rhs, u), known_vals=diff[b, 0][k[b]])
        assert not (R.unreached(k[b], d[b]) & ~k[b]).any()
    cap = 2 * max(steps)
    out, out64, res, it, cv = solve(hip, dst, k.astype(np.uint8), d.astype(np.uint8), [cap], minus=src)
    corr = out64 - src.astype(np.float64)      # the bound is about the correction this file can evaluate; subtracting src back costs one rounding of the sum
    check_planes(planes, diff, out, corr, res, it, cv, cap, f"seamless partial={partial}")
    want = np.stack([R.seamless(src[b, 0], dst[b, 0], mask[b], None if known is None else known[b]) for b in range(B)])[:, None]
    unknown = np.stack([planes[b, 0]["unk"] for b in range(B)])[:, None]
    slack = max(p["kappa"] * (2 * TOL + EPS_ROW * 4.0) for p in planes.values()) + 2 * 2.0 ** -53 * np.abs(want).max()      # the two rounded sums src + c
    assert np.abs(out64 - want)[unknown].max() <= slack and np.array_equal(out64[~unknown], dst.astype(np.float64)[~unknown])
    got, info = inpaint.blend_seamless(dev(src), dev(dst), dev(mask), known=None if known is None else dev(known), guess="zero", max_iter=cap, return_info=True)
    assert np.array_equal(bits(host(got)), bits(out)) and bool(info[2].all())
    assert np.array_equal(bits(host(got))[~unknown], bits(dst)[~unknown])      # known pixels and everything outside mask | known: dst bit for bit
    same = inpaint.blend_seamless(dev(dst), dev(dst), dev(mask), known=None if known is None else dev(known))
    assert np.abs(host(same) - dst).max() <= 1e-6 and np.array_equal(bits(host(same))[~unknown], bits(dst)[~unknown])
    one = inpaint.blend_seamless(src[0, 0], dst[0, 0], mask[0], known=None if known is None else known[0], guess="zero", max_iter=cap)      # numpy, [h, w]
    assert np.array_equal(bits(host(one)), bits(out[0, 0]))


RAW_CASE = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
AM_CASE = dict(kind="amodal", encoder="vits", guide_type="mask+observation", loss="entire_target_object")
FIELDS = ("base", "amodal", "blended", "masks", "scale_shift")
S = 70


def test_amodal_infer_image_seamless(hip):
    from _cases import build_product_model, synth_state_dict
    from hip_ext.image import masks_to_tensor
    from hip_ext.pipeline import amodal_infer_image
    raw, am = build_product_model(RAW_CASE), build_product_model(AM_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    am.load_state_dict(synth_state_dict(am), strict=True)
    raw, am = raw.cuda(), am.cuda()
    h, w = 96, 128
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(128 + 100 * np.sin(yy[..., None] * 0.07 + xx[..., None] * np.array([0.05, 0.11, 0.02])) + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    masks = np.zeros((3, h, w), np.uint8)
    masks[0] = (((yy - 40) / 25.0) ** 2 + ((xx - 70) / 30.0) ** 2 <= 1) * 255
    masks[1, :35, 80:] = 255
    masks[2, 60:90, 10:40] = 255
    masks[2, 5:12, 5:12] = 255      # a second part of object 2 that no visible pixel reaches: the plain paste there
    visible = masks.copy()
    visible[0, 40:] = 0             # the lower half is hidden
    visible[1, :, 100:] = 0
    visible[2, :, 25:] = 0
    visible[2, 5:12, 5:12] = 0
    visible[1, 60, 60] = 255        # visible outside the amodal mask: counts for nothing in the blend
    plain = amodal_infer_image(raw, am, img, masks, visible_masks=visible, size=S)
    paste = amodal_infer_image(raw, am, img, masks, visible_masks=visible, size=S, blend="paste")
    for f in FIELDS:
        assert host(getattr(plain, f)).tobytes() == host(getattr(paste, f)).tobytes(), f
    got = amodal_infer_image(raw, am, img, masks, visible_masks=visible, size=S, blend="seamless")
    for f in ("base", "amodal", "masks", "scale_shift"):
        assert host(getattr(got, f)).tobytes() == host(getattr(plain, f)).tobytes(), f
    base, pred, ss = host(got.base), host(got.amodal), host(got.scale_shift)
    m = host(got.masks) > 0
    vis = (host(masks_to_tensor(visible, S, "cuda")).reshape(3, S, S) > 0) & m
    blended = host(got.blended)
    assert blended.dtype == F and m.any(axis=(1, 2)).all() and vis.any(axis=(1, 2)).all()
    for k in range(3):
        aligned = (pred[k] * ss[k, 0] + ss[k, 1]).astype(F)      # numpy rounds the product and the sum on their own, as the kernel does
        assert np.array_equal(bits(blended[k])[~m[k]], bits(base)[~m[k]]) and np.array_equal(bits(blended[k])[vis[k]], bits(base)[vis[k]])
        diff = np.where(vis[k], base.astype(np.float64) - aligned.astype(np.float64), 0.0)
        A, rhs, unk = R.system(diff, vis[k], m[k])
        c_ref = R.solve_direct(A, rhs)
        un = R.unreached(vis[k], m[k]) & ~vis[k]
        assert np.array_equal(bits(blended[k])[un], bits(aligned)[un]) and un.any() == (k == 2)
        want = aligned.astype(np.float64)[unk] + c_ref
        # the solve stops at a recurrence residual <= 1e-9 and the true one differs from it by the recurrence's drift, orders of magnitude below that: 2e-9
        # covers it; the direct solve's residual is evaluated; the sum pred' + c is rounded to fp32 once
        bound = R.kappa(A) * (2e-9 + R.residual(A, rhs, c_ref) + EPS_ROW * np.abs(diff).max()) + 2.0 ** -24 * np.abs(want).max() * 1.0000001
        err = np.abs(blended[k][unk].astype(np.float64) - want).max()
        print(f"object {k}: unknowns {unk.sum()} kappa {R.kappa(A):.3g} err {err:.3g} bound {bound:.3g}")
        assert unk.sum() > 20 and err <= bound
        seam = np.abs(blended[k][unk] - host(plain.blended)[k][unk]).max()
        assert seam > 0      # it is not the paste
    out = amodal_infer_image(raw, am, img, masks, visible_masks=visible, size=S, blend="seamless", out_size="image", render=True)
    assert out.blended.shape == (3, h, w) and bool(torch.isfinite(out.blended).all())


def ramp_view(geometry):
    h, w = 24, 32
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (2.0 + 0.05 * xx + 0.02 * yy).astype(F)
    mask = np.ones((h, w), np.uint8)
    mask[6:15, 9:22] = 0
    photo = np.random.default_rng(2432).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return geometry.render_mesh(geometry.depth_to_mesh(depth, mask=mask, colors=photo), h, w, out="w")


def test_fill_view_and_remove_objects_harmonic(hip):
    from hip_ext import geometry, inpaint
    view = ramp_view(geometry)
    hole = host(view.owner) < 0
    assert 50 < hole.sum() < hole.size // 2
    filled = geometry.fill_view(view, method="harmonic")
    assert isinstance(filled, geometry.View) and filled.index is view.index and filled.owner is view.owner
    assert torch.equal(filled.depth.view(torch.int32), inpaint.fill_harmonic(view.depth, view.owner >= 0).view(torch.int32))
    assert torch.equal(filled.color, inpaint.fill_harmonic(view.color, view.owner >= 0))
    d = host(filled.depth)
    assert np.array_equal(bits(d)[~hole], bits(host(view.depth))[~hole]) and np.array_equal(host(filled.color)[~hole], host(view.color)[~hole])
    want = R.fill(host(view.depth), ~hole)
    assert np.abs(d - want).max() <= 2e-9 * R.kappa(R.system(host(view.depth), ~hole)[0]) + 2.0 ** -24 * np.abs(want).max()      # as in the amodal test
    lo, hi = host(view.depth)[~hole].min(), host(view.depth)[~hole].max()
    assert d[hole].min() >= lo and d[hole].max() <= hi      # the maximum principle: no hole keeps the background's 0
    depth = (np.random.default_rng(4048).integers(0, 9, (40, 48)) / 4.0 + 1.0).astype(F)
    masks = np.zeros((40, 48), np.uint8)
    masks[5:14, 7:20] = 255
    got, none = geometry.remove_objects(depth, masks, grow=0, method="harmonic")
    assert none is None and torch.equal(got.view(torch.int32), inpaint.fill_harmonic(depth, masks == 0).view(torch.int32))
    assert np.array_equal(bits(host(got))[masks == 0], bits(depth)[masks == 0])


def test_depth_to_view_fill_holes_harmonic(hip, tmp_path):
    from PIL import Image
    from hip_ext import geometry
    from hip_ext import image as hip_image
    from src.scripts import depth_to_view as S_
    h, w = 24, 32
    rng = np.random.default_rng(2432)
    depth16 = (np.where(np.arange(w)[None, :] < w // 2, 2000, 6000) + rng.integers(-50, 50, (h, w))).astype(np.uint16)
    Image.fromarray(depth16).save(tmp_path / "d.png")
    args = [str(tmp_path / "d.png"), "--max_ratio", "2", "--yaw", "12"]
    assert S_.main(args[:1] + [str(tmp_path / "smooth.png")] + args[1:] + ["--fill_holes", "smooth"]) == 0
    assert S_.main(args[:1] + [str(tmp_path / "harmonic.png")] + args[1:] + ["--fill_holes", "harmonic"]) == 0
    smooth, harmonic = (np.asarray(Image.open(tmp_path / f"{n}.png")) for n in ("smooth", "harmonic"))
    depth = depth16.astype(F)
    mesh = geometry.depth_to_mesh(depth, max_ratio=2.0)
    Rm, t = geometry.look_at_pose(12.0, 0.0, (0.0, 0.0, 0.0), pivot_z=S_.pivot_depth(depth))
    view = geometry.render_mesh(mesh, h, w, R=Rm, t=t, out="w", fill=S_.INVALID)
    hole = host(view.owner) < 0
    assert hole.sum() > 10
    for pic, method in ((smooth, "smooth"), (harmonic, "harmonic")):      # the smooth run writes the bytes it wrote before the new choice existed
        want = host(hip_image.colorize(geometry.fill_view(view, method).depth, invalid_val=S_.INVALID)[0, :, :, :3])
        assert pic.dtype == np.uint8 and np.array_equal(pic, want) and not (pic == 128).all(axis=2)[hole].any()
    assert not np.array_equal(smooth, harmonic)
