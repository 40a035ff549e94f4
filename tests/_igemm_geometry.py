"""Index arithmetic of ada_igemm, restated in closed form ("Geometry sweeps"; csrc/ada_igemm.hip).

Source side: the 3x3 walk's a_row_base (two divisions, a stride, the pitched Hp / Wp) and the tap union of an N-tile under tap_cols / tap_mask.
Destination side: the row maps (MAP_PAD, MAP_TOKEN, MAP_SHUFFLE), the epilogue's choice among its five branches, and a lane-level emulation of the
two PadWalk users (pad_start once per lane and 32-row block, pad_step by the rows-per-access of the tile's epilogue group).  Everything is plain
integer arithmetic on torch int64 tensors: no kernel, no GPU.  `Rules` switches single restatements to a plausible wrong form; the CPU test
(tests/test_igemm_geometry_cpu.py) asserts that every such mutant moves a source or destination index of at least one listed case, i.e. that the
case list would notice it, and that the case list fills the (tile, branch, map) grid.  tests/test_gpu_igemm_geometry.py runs the same list on the
device against fp64 convolutions / products of exactly representable inputs (tests/_exact.py), bit for bit, every output buffer guarded.

`walk="present"` is the rule the library had before this sweep (fast path for map_w >= 8 whatever the step); "fixed" bounds map_w by the step."""
import dataclasses
import functools

import torch
import torch.nn.functional as F

import _exact as X

C = 64                       # channels of every source: one k-step per tap, K = 576 (conv) or 64 (plain)
SENTINEL = 1024.0            # borders, cls rows, guard columns, guard images: must come back bit for bit
NAN = float("nan")           # what a launch must overwrite (outputs) or never read (sources)
BRANCHES = ("interior_op", "interior_f32res", "general_op8", "general_4col", "tail")
MAPS = ("PLAIN", "PAD", "TOKEN", "SHUFFLE")


@dataclasses.dataclass(frozen=True)
class Tile:
    cfg: int
    variant: int             # 4: single-barrier 8-wave loop, 16: generated 4-wave loop (256x256 only)
    BM: int
    BN: int
    WM: int
    WN: int

    @property
    def GW(self):            # columns per epilogue group: 64, or 32 where a wave's tile is 32 columns wide
        return 64 if self.BN // (self.WN * 32) >= 2 else 32

    @property
    def step_op(self):       # rows per wave-wide access of the operand-only paths (8 columns per lane)
        return 512 // self.GW

    @property
    def step_f32(self):      # ... of the fp32 / residual paths (4 columns per lane)
        return 256 // self.GW


TILES = {"0": Tile(0, 4, 256, 32, 4, 1), "1": Tile(1, 4, 128, 64, 4, 1), "2": Tile(2, 4, 256, 128, 4, 2), "3w8": Tile(3, 4, 256, 256, 2, 4),
         "3w4": Tile(3, 16, 256, 256, 2, 2), "4": Tile(4, 4, 128, 128, 2, 2)}


@dataclasses.dataclass(frozen=True)
class Rules:
    walk: str = "fixed"
    swap_div: bool = False            # dWo and dHoWo swapped in a_row_base
    no_image_skip: bool = False       # the 2 * (map_w + 2) rows between two images of a padded grid left out
    ignore_stride: bool = False
    wp_from_wo: bool = False          # Wp taken as Wo + 2
    shuffle_swap_ij: bool = False
    token_no_b: bool = False
    taps_first_phase: bool = False    # tap union of an N-tile from its first phase only


BASE = Rules()
PRESENT = Rules(walk="present")
MUTANTS = {
    "single-wrap step at step 16": PRESENT,
    "swapped dWo / dHoWo": Rules(swap_div=True),
    "image-border skip 2 * (map_w + 2) left out": Rules(no_image_skip=True),
    "stride ignored in a_row_base": Rules(ignore_stride=True),
    "Wp taken as Wo + 2 on a pitched input": Rules(wp_from_wo=True),
    "shuffle_row with i and j swapped": Rules(shuffle_swap_ij=True),
    "token row without + b": Rules(token_no_b=True),
    "tap union of an N-tile from its first phase only": Rules(taps_first_phase=True),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------------------------------------------------
def src_pixel(m, conv, rules=BASE):
    """Pixel index (row of the [.., Hp, Wp, lda] source) of tap (0, 0) of GEMM row m; tap t = 3 dy + dx adds dy * Wp + dx."""
    Ho, Wo, Hp, Wp, stride = conv
    if rules.swap_div:
        b, rem = m // Wo, m % Wo
        y, x = rem // (Ho * Wo), rem % (Ho * Wo)
    else:
        b, rem = m // (Ho * Wo), m % (Ho * Wo)
        y, x = rem // Wo, rem % Wo
    st = 1 if rules.ignore_stride else stride
    wp = Wo + 2 if rules.wp_from_wo else Wp
    return (b * Hp + y * st) * wp + x * st


def pad_row(m, h, w, rules=BASE):
    """Row of the zero-bordered [B, h + 2, w + 2] grid that holds pixel m."""
    b, rem = m // (h * w), m % (h * w)
    y, x = rem // w, rem % w
    if rules.no_image_skip:
        return (b * h + y + 1) * (w + 2) + x + 1
    return (b * (h + 2) + y + 1) * (w + 2) + x + 1


def token_row(m, Np, rules=BASE):
    return m + (0 if rules.token_no_b else m // Np) + 1


def shuffle_dest(m, n, h, w, s, c, rules=BASE):
    """(row [M, N] of the zero-bordered fine grid, column [N]) of GEMM element (m, n), n = (i s + j) c + co."""
    ij, co = n // c, n % c
    i, j = ij // s, ij % s
    if rules.shuffle_swap_ij:
        i, j = j, i
    b, rem = m // (h * w), m % (h * w)
    y, x = rem // w, rem % w
    row = (b[:, None] * (s * h + 2) + (s * y[:, None] + i[None, :] + 1)) * (s * w + 2) + (s * x[:, None] + j[None, :] + 1)
    return row, co


def tap_set(n0, BN, N, tap_cols, masks, rules=BASE):
    """9-bit union of the tap masks of the phases that the N-tile [n0, n0 + BN) touches."""
    first, last = n0 // tap_cols, (min(n0 + BN, N) - 1) // tap_cols
    if rules.taps_first_phase:
        last = first
    out = 0
    for ph in range(first, last + 1):
        out |= masks[ph]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    family: str
    tile: str
    B: int
    N: int
    want: str                         # the branch this case is meant to reach on at least one of its tiles
    out: str = "op"                   # "op", "f32", "f32+op", "tail"
    map_op: str = "PLAIN"
    map_f32: str = "PLAIN"
    map_h: int = 0
    map_w: int = 0
    conv: tuple = None                # (Ho, Wo, Hp, Wp, stride); None: plain A, K = 64
    HW: tuple = None                  # the convolution's input grid (H, W)
    res: bool = False
    relu: bool = False
    ldo_op: int = 0
    ldo_f32: int = 0
    split: int = 0                    # +1: [hi | lo], -1: [hi | lo8 | hi8]; the segment is N wide
    s: int = 0                        # shuffle / sub-pixel factor
    c: int = 0                        # shuffle_c, or tap_cols of the masked walk
    Np: int = 0

    @property
    def M(self):
        if self.conv:
            return self.B * self.conv[0] * self.conv[1]
        return self.B * (self.Np if self.Np else self.map_h * self.map_w)

    @property
    def K(self):
        return 9 * C if self.conv else C

    @property
    def has_op(self):
        return "op" in self.out

    @property
    def has_f32(self):
        return "f32" in self.out or self.out == "tail"

    @property
    def cell_map(self):
        return self.map_op if (self.has_op and self.map_op != "PLAIN") else (self.map_f32 if self.has_f32 else "PLAIN")

    @property
    def masked(self):
        return self.family == "taps"

    @property
    def id(self):
        g = f"Np{self.Np}" if self.Np else (f"{self.map_h}x{self.map_w}" if self.map_h else "")
        src = "" if not self.conv else f"-in{self.HW[0]}x{self.HW[1]}p{self.conv[2]}x{self.conv[3]}s{self.conv[4]}"
        extra = (f"-s{self.s}c{self.c}" if self.s else "") + (f"-split{self.split}" if self.split else "") + (f"-ld{self.ldo_op}" if self.has_op else "")
        return f"{self.family}-t{self.tile}-{self.out}-{self.cell_map}{g}{src}-B{self.B}-N{self.N}{extra}"


def tiles_of(case):
    t = TILES[case.tile]
    return [(m0, n0) for m0 in range(0, case.M, t.BM) for n0 in range(0, case.N, t.BN)]


def branch(case, m0, n0, rules=BASE):
    """The epilogue branch of tile (m0, n0): the `if` chain of igemm_kernel behind the main loop, for the STD / SHUFFLE / TAIL epilogues."""
    t = TILES[case.tile]
    if case.out == "tail":
        return "tail"
    shuffle = case.has_op and case.map_op == "SHUFFLE"
    op_only = not case.has_f32 and not case.res
    bound = 8 if rules.walk == "present" else (t.step_op if op_only else t.step_f32)
    interior = (not shuffle and m0 + t.BM <= case.M and n0 + t.BN <= case.N and not case.Np
                and (not case.has_op or case.map_op == "PLAIN" or (case.map_op == "PAD" and case.map_w >= bound))
                and (not case.has_f32 or case.map_f32 == "PLAIN")
                and (case.has_f32 or case.res or case.ldo_op % 8 == 0))
    if interior:
        return "interior_op" if op_only else "interior_f32res"
    if op_only and case.ldo_op % 8 == 0 and (not shuffle or case.c % 8 == 0):
        return "general_op8"
    return "general_4col"


def branches(case, rules=BASE):
    return {branch(case, m0, n0, rules) for m0, n0 in tiles_of(case)}


def emulated_pad_rows(case, rules=BASE):
    """[N-tiles, M]: the padded-grid row every GEMM row of every tile is stored to, lane by lane.  On the interior branches each lane rsub < step of
    each wave starts a PadWalk at the first row of each 32-row block it owns (pad_start: two divisions) and advances it `step` rows per store with
    pad_step's single wrap of x; the general branches evaluate the closed form per row."""
    t = TILES[case.tile]
    h, w, M = case.map_h, case.map_w, case.M
    n_tiles = list(range(0, case.N, t.BN))
    out = torch.full((len(n_tiles), M), -1, dtype=torch.int64)
    closed = pad_row(torch.arange(M), h, w)
    for tn, n0 in enumerate(n_tiles):
        for m0 in range(0, M, t.BM):
            br = branch(case, m0, n0, rules)
            if not br.startswith("interior"):
                hi = min(m0 + t.BM, M)
                out[tn, m0:hi] = closed[m0:hi]
                continue
            step = t.step_op if br == "interior_op" else t.step_f32
            for blk in range(m0, m0 + t.BM, 32):          # (wave, i) -> one 32-row block each
                for rsub in range(step):
                    m = blk + rsub
                    b, rem = divmod(m, h * w)
                    y, x = divmod(rem, w)
                    prow = (b * (h + 2) + y + 1) * (w + 2) + x + 1
                    for k in range(32 // step):
                        out[tn, m + k * step] = prow
                        x += step
                        prow += step
                        if x >= w:
                            x -= w
                            y += 1
                            prow += 2
                            if y >= h:
                                y = 0
                                prow += 2 * (w + 2)
    assert int(out.min()) >= 0
    return out


emulated_pad_rows = functools.lru_cache(maxsize=None)(emulated_pad_rows)


def indices(case, rules=BASE):
    """Every source and destination index of a case under `rules`, as a list of int64 tensors: what a mutant must move to be noticed."""
    m = torch.arange(case.M)
    out = []
    if case.conv:
        out.append(src_pixel(m, case.conv, rules))
    if case.masked:
        masks = X.subpixel_masks(case.s)
        out.append(torch.tensor([tap_set(n0, TILES[case.tile].BN, case.N, case.c, masks, rules) for n0 in range(0, case.N, TILES[case.tile].BN)]))
    if case.has_op and case.map_op == "PAD":
        walked = emulated_pad_rows(case, Rules(walk=rules.walk))
        out.append(pad_row(m, case.map_h, case.map_w, rules).expand_as(walked) if rules.no_image_skip else walked)
    if "TOKEN" in (case.map_op, case.map_f32):
        out.append(token_row(m, case.Np, rules))
    if case.map_op == "SHUFFLE":
        out.append(shuffle_dest(m, torch.arange(case.N), case.map_h, case.map_w, case.s, case.c, rules)[0])
    return out


def im2col(case, buf, rules=BASE, taps=0x1ff):
    """[M, 9 C] rows gathered from the source buffer by the restated walk; taps outside `taps` are left zero (the masked walk never stages them)."""
    flat = buf.reshape(-1, C)
    base = src_pixel(torch.arange(case.M), case.conv, rules)
    wp = case.conv[3]
    out = torch.zeros(case.M, 9, C, dtype=buf.dtype)
    for t in range(9):
        if (taps >> t) & 1:
            out[:, t] = flat[base + (t // 3) * wp + t % 3]
    return out.reshape(case.M, 9 * C)


def _batch(hw, bm, rows=2):
    """Images so that M = B hw lies just above `rows` tile rows and ends in a ragged tile."""
    B = max(2, -(-(rows * bm + 1) // hw))
    while (B * hw) % bm == 0:
        B += 1
    return B


MAP_WIDTHS = (1, 2, 3, 4, 7, 8, 9, 12, 15, 16, 17, 31, 33)      # both sides of every walk step (4, 8, 16); 4 itself, the fp32 half's step on 64-column groups
MAP_HEIGHTS = (1, 2, 5)
TINY = ((1, 1), (1, 2), (2, 2), (2, 9), (8, 8), (9, 8), (16, 15))


def _pad_cases():
    out = []
    for ti, (key, t) in enumerate(TILES.items()):
        for wi, w in enumerate(MAP_WIDTHS):
            # the widths next to a step get every height; the others rotate
            heights = MAP_HEIGHTS if w in (7, 8, 9, 15, 16, 17) and key in ("0", "3w8") else (MAP_HEIGHTS[(wi + ti) % 3],)
            for hi_, h in enumerate(heights):
                B = _batch(h * w, t.BM)
                N = (t.BN, t.BN + 8, 2 * t.BN)[(wi + hi_) % 3 if w not in (9, 12) else 0]
                conv = (h, w, h + 2, w + 2, 1)
                geo = dict(tile=key, B=B, N=N, map_h=h, map_w=w, conv=conv, HW=(h, w), relu=True)
                out.append(Case("pad_op", want="interior_op" if w >= t.step_op else "general_op8", map_op="PAD", ldo_op=N + 8, **geo))
                if hi_ == 0:
                    out.append(Case("pad_f32res", want="interior_f32res" if w >= t.step_f32 else "general_4col", out="f32+op", res=True, map_op="PAD",
                                    ldo_op=N + 8, ldo_f32=N + 4, **geo))
                if hi_ == 0 and w in (7, 9, 16):
                    out.append(Case("pad_op", want="general_4col", map_op="PAD", ldo_op=N + 4, **geo))
        # split stores share the walked address: both forms, on both PadWalk users, next to the steps
        for w, h, split, f32 in ((9, 5, 1, False), (16, 2, -1, False), (12, 1, 1, True), (7, 5, -1, True), (3, 2, 1, True), (7, 2, 1, False), (15, 1, -1, False)):
            B = _batch(h * w, t.BM)
            geo = dict(tile=key, B=B, N=t.BN, map_h=h, map_w=w, conv=(h, w, h + 2, w + 2, 1), HW=(h, w), relu=True, split=split, ldo_op=2 * t.BN + 8)
            if f32:
                out.append(Case("pad_split", want="interior_f32res" if w >= t.step_f32 else "general_4col", out="f32+op", res=True, map_op="PAD", ldo_f32=t.BN + 4, **geo))
            else:
                out.append(Case("pad_split", want="interior_op" if w >= t.step_op else "general_op8", map_op="PAD", **geo))
    return out


def _conv_geo(H, W, stride, pitched):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Hp, Wp = (Ho - 1) * stride + 3, (Wo - 1) * stride + 3
    if pitched:
        Hp, Wp = Hp + 2, Wp + 3
    return Ho, Wo, Hp, Wp


def _stride2_cases():
    out = []
    for ti, key in enumerate(("1", "3w8", "3w4")):
        t = TILES[key]
        for gi, (H, W) in enumerate(TINY):
            for oi, kind in enumerate(("op", "f32")):
                Ho, Wo, Hp, Wp = _conv_geo(H, W, 2, pitched=(gi + oi + ti) % 2 == 1)
                B = max(3, -(-(t.BM + 40) // (Ho * Wo)))
                geo = dict(tile=key, B=B, N=64, conv=(Ho, Wo, Hp, Wp, 2), HW=(H, W))
                if kind == "op":
                    out.append(Case("stride2", want="general_op8", map_op="PAD", map_h=Ho, map_w=Wo, relu=True, ldo_op=72, **geo))
                else:
                    out.append(Case("stride2", want="general_4col", out="f32", ldo_f32=68, **geo))
    return out


def _pitched_cases():
    out = []
    for ti, (key, t) in enumerate(TILES.items()):
        for gi, (H, W) in enumerate(TINY):
            Ho, Wo, Hp, Wp = _conv_geo(H, W, 1, pitched=True)
            geo = dict(tile=key, B=_batch(H * W, t.BM), N=t.BN, conv=(Ho, Wo, Hp, Wp, 1), HW=(H, W))
            if (gi + ti) % 2 == 0:
                out.append(Case("pitched", want="interior_op", relu=True, ldo_op=t.BN + 8, **geo))
            else:
                out.append(Case("pitched", want="interior_f32res", out="f32", res=True, ldo_f32=t.BN + 4, **geo))
    for key in ("0", "1"):                                   # the tail epilogue picks its own tile: N <= 32 -> 256x32, else 128x64
        for H, W in ((1, 1), (2, 9), (9, 8)):
            Ho, Wo, Hp, Wp = _conv_geo(H, W, 1, pitched=True)
            out.append(Case("tail", tile=key, B=_batch(H * W, TILES[key].BM), N=TILES[key].BN, want="tail", out="tail", ldo_f32=1, conv=(Ho, Wo, Hp, Wp, 1), HW=(H, W)))
    return out


SHUFFLE_GRIDS = ((1, 1), (1, 9), (3, 2), (8, 8), (5, 13))


def _shuffle_cases():
    out = []
    for ti, (key, t) in enumerate(TILES.items()):
        for gi, (h, w) in enumerate(SHUFFLE_GRIDS):
            for ci, c in enumerate((8, 48, 12)):
                s = (2, 4)[(gi + ci + ti) % 2]
                out.append(Case("shuffle", tile=key, B=_batch(h * w, t.BM, rows=1), N=s * s * c, want="general_4col" if c % 8 else "general_op8", map_op="SHUFFLE",
                                map_h=h, map_w=w, s=s, c=c, ldo_op=c + 8))
    return out


def _token_cases():
    out = []
    for key, t in TILES.items():
        for Np in (1, 2, 255, 256, 257):
            B = 3 if Np >= 255 else _batch(Np, t.BM, rows=1)
            out.append(Case("token", tile=key, B=B, N=64, Np=Np, map_h=Np, want="general_4col", out="f32", res=True, map_f32="TOKEN", ldo_f32=68))
            out.append(Case("token", tile=key, B=B, N=64, Np=Np, map_h=Np, want="general_op8", map_op="TOKEN", ldo_op=72))
    return out


def _tap_cases():
    out = []
    # (tile, tap_cols): the N-tile spans one phase (256x32 over 32-column phases), several, and -- where s s tap_cols <= BN -- all of them
    for key, co in (("0", 32), ("0", 16), ("1", 16), ("2", 16), ("3w8", 16), ("4", 16)):
        for s in (2, 4):
            for H, W in ((1, 1), (1, 2), (2, 1), (3, 8)):
                out.append(Case("taps", tile=key, B=12 if H * W > 2 else 3, N=s * s * co, want="general_4col", out="f32", ldo_f32=s * s * co + 4, s=s, c=co,
                                conv=(H, W, H + 2, W + 2, 1), HW=(H, W)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_pad_cases() + _stride2_cases() + _pitched_cases() + _shuffle_cases() + _token_cases() + _tap_cases())


def by_family(*families):
    return [c for c in cases() if c.family in families]


# cells of the (tile, branch, map) grid that no launch can reach, with the reason
def impossible(tile, br, mp):
    if br == "tail":
        if tile not in ("0", "1"):
            return "the tail epilogue (N <= 64) is built for the 256x32 and 128x64 tiles only"
        if mp != "PLAIN":
            return "the tail epilogue writes one fp32 value per GEMM row, unmapped"
        return None
    if br.startswith("interior") and mp in ("TOKEN", "SHUFFLE"):
        return "the interior fast path takes plain and padded row maps only (token rows and shuffled rows go through the general paths)"
    return None
# (the SwiGLU epilogue -- 128x128 and 256x256 tiles only, MAP_PLAIN only -- has one branch of its own and no row map: it is not part of this grid)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact inputs and the fp64 values
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows(t, n):
    return t.permute(0, 2, 3, 1).reshape(-1, n)


@functools.lru_cache(maxsize=None)
def conv_data(B, H, W_, Co, stride):
    c = X.conv_family(B, C, H, W_, Co, seed=50 + stride)
    x, w, b = c["x"], c["w"], c["bias"]
    lin = _rows(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1), Co)
    mag = _rows(F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=stride, padding=1), Co)
    res = X.fp32_dyadic((lin.shape[0], Co), 4096, 64, 52)
    orders = lambda: [_rows(F.conv2d(x, w, b, stride=stride, padding=1), Co), _rows(F.conv2d(x.flip(1), w.flip(1), b, stride=stride, padding=1), Co)]      # noqa: E731
    return dict(x=x, W=w.permute(0, 2, 3, 1).reshape(Co, 9 * C).contiguous(), bias=b, res=res, lin=lin, mag=mag, unit=c["unit"], orders=orders)


def source_buffer(x, conv):
    """[B + 1, Hp, Wp, C] fp32: the zero-bordered NHWC map in the corner a correct walk reads, NaN in every pitch row / column and in an extra image."""
    B, _, H, W_ = x.shape
    Ho, Wo, Hp, Wp, stride = conv
    nh, nw = (Ho - 1) * stride + 3, (Wo - 1) * stride + 3
    full = torch.zeros(B, H + 2, W_ + 2, C)
    full[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    buf = torch.full((B + 1, Hp, Wp, C), NAN)
    buf[:B, :nh, :nw] = full[:, :nh, :nw]
    return buf


@functools.lru_cache(maxsize=None)
def data_key(case):
    """What the inputs of a case depend on: cases that share it share tensors."""
    if case.family == "taps":
        return ("taps", case.s, case.c, case.HW, case.B)
    if case.conv:
        return ("conv", case.B, case.HW, case.N, case.conv[4], case.out == "tail")
    if case.family == "shuffle":
        return ("shuffle", case.s, case.c, case.map_h, case.map_w, case.B)
    return ("token", case.B, case.Np, case.N)


@functools.lru_cache(maxsize=None)
def _data(key):
    kind = key[0]
    if kind == "taps":
        _, s, co, (H, W_), B = key
        f = X.subpixel_family(s, C, co, H, W_, B)
        return dict(x=f["x"], W=f["wm"].reshape(-1, 9 * C).contiguous(), bias=f["bias"], lin=f["ref"], mag=_rows(f["mag"], s * s * co), unit=f["unit"], orders=f["orders"],
                    masks=tuple(f["masks"]))
    if kind == "conv":
        _, B, (H, W_), N, stride, tail = key
        d = dict(conv_data(B, H, W_, N, stride))
        if tail:
            tw = X.fp32_dyadic((N,), 8, 8, 60)
            d["tw"] = tw
            d["dot"] = (d["lin"].clamp_min(0) * tw.double()).sum(1) + 0.25
            d["dot_mag"] = (d["lin"].clamp_min(0) * tw.double().abs()).sum(1) + 0.25
            lin_orders = d["orders"]
            d["dot_orders"] = lambda: [(lin_orders()[0].clamp_min(0) * tw).sum(1) + 0.25, (lin_orders()[1].clamp_min(0).flip(1) * tw.flip(0)).sum(1) + 0.25]
        return d
    if kind == "shuffle":
        _, s, c, h, w, B = key
        f = X.shuffle_family(s, c, C, h, w, B)
        return dict(A=f["A"], W=f["Wp"], bias=f["bias"], lin=f["flat"], mag=f["mag"], unit=f["unit"], orders=f["orders"])
    _, B, Np, N = key
    f = X.small_family(B * Np, N, C, seed=70 + Np % 7)
    pos = X.fp32_dyadic((Np + 1, N), 4096, 64, 71)
    lin = f["lin"] + f["bias"].double()
    mag = f["A"].double().abs() @ f["W"].double().abs().T + f["bias"].double().abs()
    perm = X.reversed_chunks(C, 16)
    orders = lambda: [f["A"] @ f["W"].T + f["bias"], f["A"][:, perm] @ f["W"][:, perm].T + f["bias"]]      # noqa: E731
    return dict(A=f["A"], W=f["W"], bias=f["bias"], pos=pos, lin=lin, mag=mag, unit=f["unit"], orders=orders)


def data(case):
    return _data(data_key(case))


def residual(case, d):
    """[M, N] fp32 residual as the launch sees it per GEMM row (the token map reads pos[1 + m % Np])."""
    if not case.res:
        return None
    if case.Np:
        return d["pos"][1:].repeat(case.B, 1)
    return d["res"]


def values(case, d):
    """(fp64 value before the per-copy ReLU, budget magnitude)."""
    r = residual(case, d)
    if r is None:
        return d["lin"], d["mag"]
    return d["lin"] + r.double(), d["mag"] + r.double().abs()


def a_buffer(case, d):
    return source_buffer(d["x"], case.conv) if case.conv else d["A"]


# ---------------------------------------------------------------------------------------------------------------------------------
# guarded output buffers and what they must hold afterwards
# ---------------------------------------------------------------------------------------------------------------------------------
def _prefill(case, mp, ld, ncols):
    """fp32 [rows, ld]: NaN where the launch must write, SENTINEL in borders / cls rows / guard columns and in one whole guard image behind the last."""
    B = case.B
    if mp == "PAD" or mp == "SHUFFLE":
        s = case.s if mp == "SHUFFLE" else 1
        t = torch.full((B + 1, s * case.map_h + 2, s * case.map_w + 2, ld), SENTINEL)
        t[:B, 1:-1, 1:-1, :ncols] = NAN
    elif mp == "TOKEN":
        t = torch.full((B + 1, case.Np + 1, ld), SENTINEL)
        t[:B, 1:, :ncols] = NAN
    else:
        t = torch.full((case.M + 8, ld), SENTINEL)
        t[:case.M, :ncols] = NAN
    return t.reshape(-1, ld)


def dest_rows(case, mp):
    m = torch.arange(case.M)
    if mp == "PAD":
        return pad_row(m, case.map_h, case.map_w)
    if mp == "TOKEN":
        return token_row(m, case.Np)
    return m


def op_prefill(case):
    ncols = case.c if case.map_op == "SHUFFLE" else (2 * case.N if case.split else case.N)
    return _prefill(case, case.map_op, case.ldo_op, ncols)


def f32_prefill(case):
    if case.out == "tail":
        t = torch.full((case.M + 8, 1), SENTINEL)
        t[:case.M] = NAN
        return t
    return _prefill(case, case.map_f32, case.ldo_f32, case.N)


def expected_f32(case, v64):
    buf = f32_prefill(case)
    want = v64.float()
    assert torch.equal(want.double(), v64)
    if case.out == "tail":
        buf[:case.M, 0] = want
    else:
        buf[dest_rows(case, case.map_f32), :case.N] = want
    return buf


def expected_op(case, v64, op):
    """The operand-typed buffer after the launch, in `op` -- or as bytes [rows, 2 ldo_op] for the [hi | lo8 | hi8] form."""
    N = case.N
    v = v64.clamp_min(0) if case.relu else v64
    buf = op_prefill(case).to(op)
    if case.map_op == "SHUFFLE":
        rows, cols = shuffle_dest(torch.arange(case.M), torch.arange(N), case.map_h, case.map_w, case.s, case.c)
        buf[rows, cols[None, :].expand_as(rows)] = X.rne(v, op)
        return buf
    rows = dest_rows(case, case.map_op)
    if case.split == 0:
        buf[rows, :N] = X.rne(v, op)
    elif case.split > 0:
        hi, lo = X.split_ref(v, op)
        assert torch.equal(hi.double() + lo.double(), v)
        buf[rows, :N], buf[rows, N:2 * N] = hi, lo
    else:
        assert op == torch.float16
        hi = X.rne(v, op)
        resid = (v - hi.double()) * 1024.0
        assert torch.equal(resid.float().double(), resid)
        raw = buf.view(torch.uint8).reshape(buf.shape[0], 2 * case.ldo_op).clone()
        raw[rows, :2 * N] = hi.contiguous().view(torch.uint8).reshape(-1, 2 * N)
        raw[rows, 2 * N:3 * N] = X.e5m2(resid.float())
        raw[rows, 3 * N:4 * N] = X.e5m2(v.float())
        return raw
    return buf
