"""Geometries, inputs and references for the kernels that turn token rows into an image and back - the fused un-embed
(cra5_gemm_nt_split_unembed, its side buffer and fix-up), the overlap-add (col2im, generic and LDS-tiled) and the patch
gather (im2col, generic and LDS-tiled) - away from the model's 72 x 144 token grid.  Shared by
tests/test_patch_geometry_gpu.py (the kernels) and tests/test_patch_geometry_inputs_cpu.py (these helpers themselves).

A subset decode launches these kernels on the superset geometry subset.token_plan returns: n_ti token rows (1 .. 72) by
n_tj token columns (even, 2 .. 144), image [C, 10 n_ti + 1, 10 n_tj].  CASES is the list of geometries the GPU tests
run; geometry_classes() names what can differ between two geometries inside the kernels (rows of the un-embed GEMM's
256-row tile and 32-row sub-tile, seams, which col2im / im2col kernel the launcher picks, 16-token tiles per row), and
the CPU tests prove that every class a reachable superset belongs to is one some case belongs to.

The exact-arithmetic inputs, their expectations and the mismatch report come from exact_helpers; the split-f16 store's
model from split_helpers.  Nothing here calls a product kernel."""
import functools

import torch
import torch.nn.functional as F

import exact_helpers as X

KH, KW, SH, SW = 11, 10, 10, 10
GRID_HP, GRID_WP = 72, 144
GEMM_TILE_ROWS, GEMM_SUB_ROWS, GEMM_TILE_COLS = 256, 32, 256      # the un-embed launch: 256 x 256 tiles, 32-row sub-tiles
# restated from csrc/elementwise.hip
TILE_TOK = 16
TILE_CH = 2
TILE_CH_S = 2
IM2COL_GROUP = 2

U = 2.0 ** -24            # unit roundoff of fp32

# ------------------------------------------------------------------------------------------------ geometry classes

ROWS_1 = "Hp = 1: no seam row, the first patch row is the last"
ROWS_2 = "Hp = 2: one seam"
ROWS_N = "Hp >= 3: interior patch rows"
M_SUB = "M < 32: less than one 32-row sub-tile"
M_PART = "32 <= M < 256: one partial 256-row tile"
M_ONE = "M = 256: exactly one 256-row tile"
M_TAIL_SUB = "M > 256: the last tile holds less than one sub-tile"
M_TAIL = "M > 256: the last tile is partial, 32 rows or more"
M_WHOLE = "M > 256: whole tiles only"
CUT_INSIDE = "a tile boundary falls inside a token row"
CUT_BETWEEN = "tile boundaries fall between token rows"
W_THIN = "n_tj = 2: W = 20"
W_GENERIC = "n_tj % 16 != 0: generic col2im / im2col"
W_CIRCLE = "n_tj = 144: the whole circle"
TILED_HP = {1: "tiled kernels at Hp = 1", 2: "tiled kernels at Hp = 2", 3: "tiled kernels at Hp >= 3"}
TILED_W = {1: "one 16-token tile per row", 2: "two 16-token tiles per row", 3: "three 16-token tiles per row",
           4: "four or more 16-token tiles per row"}


def geometry_classes(n_ti, n_tj):
    """the classes of the superset geometry (n_ti, n_tj): one label per axis (patch rows, rows of the GEMM tile, where the
    tile boundary falls, width), two more where the LDS-tiled kernels apply"""
    assert 1 <= n_ti <= GRID_HP and 2 <= n_tj <= GRID_WP and n_tj % 2 == 0, (n_ti, n_tj)
    M = n_ti * n_tj
    out = {ROWS_1 if n_ti == 1 else ROWS_2 if n_ti == 2 else ROWS_N}
    if M < GEMM_SUB_ROWS:
        out.add(M_SUB)
    elif M < GEMM_TILE_ROWS:
        out.add(M_PART)
    elif M == GEMM_TILE_ROWS:
        out.add(M_ONE)
    else:
        tail = M % GEMM_TILE_ROWS
        out.add(M_WHOLE if tail == 0 else M_TAIL_SUB if tail < GEMM_SUB_ROWS else M_TAIL)
        out.add(CUT_BETWEEN if GEMM_TILE_ROWS % n_tj == 0 else CUT_INSIDE)
    if n_tj == 2:
        out.add(W_THIN)
    elif n_tj % TILE_TOK:
        out.add(W_GENERIC)
    else:
        out.add(TILED_HP[min(n_ti, 3)])
        out.add(TILED_W[min(n_tj // TILE_TOK, 4)])
    if n_tj == GRID_WP:
        out.add(W_CIRCLE)
    return frozenset(out)


# (n_ti, n_tj, the classes the case is in the list for)
CASES = [
    (1, 2, (ROWS_1, M_SUB, W_THIN)),
    (2, 2, (ROWS_2, M_SUB)),
    (2, 6, (ROWS_2, M_SUB, W_GENERIC)),
    (34, 2, (ROWS_N, M_PART, W_THIN)),
    (72, 2, (ROWS_N, M_PART, W_THIN)),
    (16, 16, (M_ONE, TILED_HP[3], TILED_W[1])),
    (3, 86, (M_TAIL_SUB, CUT_INSIDE, W_GENERIC)),
    (16, 30, (M_TAIL, CUT_INSIDE, W_GENERIC)),
    (1, 16, (ROWS_1, TILED_HP[1], TILED_W[1])),
    (2, 16, (ROWS_2, TILED_HP[2], TILED_W[1])),
    (3, 32, (TILED_HP[3], TILED_W[2])),
    (1, 48, (TILED_HP[1], TILED_W[3])),
    (7, 144, (W_CIRCLE, M_TAIL, CUT_INSIDE, TILED_W[4])),
    (32, 16, (M_WHOLE, CUT_BETWEEN)),
]
GEOMETRIES = [(a, b) for a, b, _ in CASES]
ALL_CLASSES = frozenset([ROWS_1, ROWS_2, ROWS_N, M_SUB, M_PART, M_ONE, M_TAIL_SUB, M_TAIL, M_WHOLE, CUT_INSIDE, CUT_BETWEEN,
                         W_THIN, W_GENERIC, W_CIRCLE]) | frozenset(TILED_HP.values()) | frozenset(TILED_W.values())

UNEMBED_CHANNELS = (1, 3, 8)          # N = 110, 330 (column 256 inside a (c, ky) run), 880
# (name, K, hi_only, plain A and W): the four instantiations of the fused launch
UNEMBED_FORMS = (("fp32-accurate", 128, False, False), ("hi_only, split rows", 128, True, False),
                 ("hi_only, split rows, Kp % 64 != 0", 96, True, False), ("hi_only, plain A and W", 128, True, True))
IM2COL_GEOMETRIES = [(1, 16), (2, 16), (3, 32), (1, 2), (2, 6), (3, 15)]
IM2COL_CHANNELS = (1, 2, 3, 4, 5)
COL2IM_CHANNELS = (1, 2, 3, 5)

# the boxes tests/test_subset_decode_gpu.py adds to BOXES: (box, (ti0, n_ti, tj0, n_tj) of its superset, why)
MODEL_BOXES = [
    ((205, 236, 403, 150), (20, 4, 40, 16), "n_tj = 16 away from the east edge"),
    ((301, 322, 1385, 155), (30, 3, 138, 16), "n_tj = 16 across the east edge"),
    ((401, 560, 800, 160), (40, 16, 80, 16), "(16, 16): M = 256, exactly one tile"),
    ((101, 130, 15, 850), (10, 3, 1, 86), "(3, 86): the second tile holds two rows"),
    ((0, 15, 640, 320), (0, 2, 64, 32), "the top edge with a tiled superset"),
    ((700, 721, 1120, 160), (69, 3, 112, 16), "the bottom edge with a tiled superset"),
]


def image_shape(n_ti, n_tj):
    return (n_ti - 1) * SH + KH, n_tj * KW


def channel_classes(C):
    """what the channel count decides inside the kernels"""
    N, n_cc = C * KH * KW, -(-C // TILE_CH)
    out = {f"{-(-N // GEMM_TILE_COLS)} tile column(s), the last one ragged"}
    if N > GEMM_TILE_COLS:
        out.add("the boundary at column 256 falls inside a (c, ky) run")
    out.add("odd C: the last channel chunk holds one channel (kpt = 110, q4 = 28), K % 4 == 2" if C % 2 else "even C: K % 4 == 0")
    out.add(f"im2col: {-(-n_cc // IM2COL_GROUP)} block(s) per token tile, the last walks {(n_cc - 1) % IM2COL_GROUP + 1} chunk(s)")
    return frozenset(out)


def kernel_choice(op, n_tj, ld, W=None, alignment=0):
    """'tiled' | 'generic': the launchers' own predicates (cra5_col2im_f32 / cra5_im2col_f32 in csrc/elementwise.hip) for
    the ERA5 patch (11, 10) / stride (10, 10).  ld: row pitch of the column matrix in floats; W: image width (col2im:
    always 10 n_tj; im2col may be wider); alignment: byte offset from a 16-byte boundary of the column matrix and of the
    image - one number for both or (cols, image)."""
    a_cols, a_img = alignment if isinstance(alignment, tuple) else (alignment, alignment)
    W = n_tj * KW if W is None else W
    ok = n_tj % TILE_TOK == 0 and W % 4 == 0 and ld % 4 == 0 and a_img % 16 == 0
    if op == "col2im":
        assert W == n_tj * KW
        ok = ok and a_cols % 16 == 0
    else:
        assert op == "im2col" and W >= n_tj * KW
    return "tiled" if ok else "generic"


def classify(n_ti, n_tj, C, ld, alignment=0, op="col2im", W=None):
    """-> dict(kernel = 'tiled' | 'generic', classes = geometry_classes | channel_classes)"""
    assert ld >= C * KH * KW
    return dict(kernel=kernel_choice(op, n_tj, ld, W, alignment), classes=geometry_classes(n_ti, n_tj) | channel_classes(C))


def padded_pitch(K):
    """K rounded up to a multiple of 4, plus 4: a pitch with which an odd channel count reaches the tiled kernels"""
    return (K + 3) // 4 * 4 + 4


# ------------------------------------------------------------------------------------------------ references


def col2im_reference(cols, C, Hp, Wp, mean=None, std=None):
    """fold of cols [Hp * Wp, C * 110] (column (c * 11 + ky) * 10 + kx) in cols' own dtype -> [C, 10 Hp + 1, 10 Wp], then
    x * std[c] + mean[c] in that dtype.  float64 in: the reference; fp32 in: the same IEEE sums a kernel makes (a
    two-term sum has one rounding in either order)."""
    H, W = image_shape(Hp, Wp)
    assert cols.shape == (Hp * Wp, C * KH * KW)
    img = F.fold(cols.t().contiguous()[None], (H, W), (KH, KW), stride=(SH, SW))[0]
    if std is not None:
        img = img * std.to(img.dtype)[:, None, None] + mean.to(img.dtype)[:, None, None]
    return img


def im2col_reference(x, Hp, Wp, mean=None, std=None):
    """unfold of x [C, H, W] (H >= 10 Hp + 1, W >= 10 Wp: rows / columns past the patches are not read) after
    (x - mean[c]) / std[c] in x's dtype -> [Hp * Wp, C * 110]"""
    if mean is not None:
        x = (x - mean.to(x.dtype)[:, None, None]) / std.to(x.dtype)[:, None, None]
    H, W = image_shape(Hp, Wp)
    assert x.shape[1] >= H and x.shape[2] >= W
    return F.unfold(x[None, :, :H, :W], (KH, KW), stride=(SH, SW))[0].t().contiguous()


def denorm_bound(s64, std, mean):
    """2 u (|s std| + |mean|) per pixel of the float64 overlap sum s64 [C, H, W].  Derived, for s an exact fp32 number
    (quantised_cols): a rounding to nearest has relative error d, |d| <= u / (1 + u).  Contracted, the kernel computes
    fl(r), r = s std + mean: error <= u |r|.  Not contracted, fl(fl(s std) + mean) = (s std (1 + d1) + mean)(1 + d2):
    error = |s std d1 (1 + d2) + r d2| <= |s std| u (1 + 2 u) / (1 + u)^2 + u |r| < u |s std| + u |r|.  With
    |r| <= |s std| + |mean| both are below 2 u |s std| + u |mean|, which the bound exceeds by u |mean|."""
    return 2.0 * U * ((s64 * std.double()[:, None, None]).abs() + mean.double().abs()[:, None, None])


# ------------------------------------------------------------------------------------------------ inputs


def exact_stats(C):
    """(mean, std) with which x * std + mean is exact on the grid data: small integers, powers of two"""
    return (torch.arange(C) % 7 - 3).float(), (2.0 ** (torch.arange(C) % 3)).float()


def random_stats(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g) * 50, torch.rand(C, generator=g) * 30 + 0.5


@functools.lru_cache(maxsize=8)
def unembed_operands(n_ti, n_tj, C, K):
    """(A [n_ti * n_tj, K], W [C * 110, K]) fp32 on the exact grid p + q 2^-12 (exact_helpers.grid_matrix, no zeros).
    Read-only: shared between the engine forms."""
    seed = 100003 * n_ti + 1009 * n_tj + 17 * C + K
    return X.grid_matrix(n_ti * n_tj, K, 1.0, seed), X.grid_matrix(C * KH * KW, K, 1.0, seed + 1)


def exact_cols(n_ti, n_tj, C, seed=0):
    """column matrix [M, C * 110] on the grid p + q 2^-12: every overlap sum and x * std + mean of exact_stats is an exact
    fp32 number"""
    return X.grid_matrix(n_ti * n_tj, C * KH * KW, 1.0, 7919 * n_ti + 31 * n_tj + C + seed)


def random_cols(n_ti, n_tj, C, seed=0):
    g = torch.Generator().manual_seed(104729 * n_ti + 37 * n_tj + C + seed)
    return torch.randn(n_ti * n_tj, C * KH * KW, generator=g)


def quantised_cols(n_ti, n_tj, C, seed=0):
    """random multiples of 2^-10 in [-4, 4]: 13 bits, so the two-term overlap sum is an exact fp32 number and the only
    roundings of the de-normalised result are those of s * std + mean (denorm_bound's premise)"""
    g = torch.Generator().manual_seed(15485863 * n_ti + 41 * n_tj + C + seed)
    return torch.randint(-4096, 4097, (n_ti * n_tj, C * KH * KW), generator=g).float() * 2.0 ** -10


def im2col_image(Hp, Wp, C, seed=0):
    """random image [C, 10 Hp + 5, 10 Wp + 4] (larger than the patches cover; Wp = 15: W = 150, W % 4 != 0) and stats"""
    H, W = SH * Hp + 5, (SW * Wp + 4 if Wp % 2 == 0 else SW * Wp)
    g = torch.Generator().manual_seed(6151 * Hp + 43 * Wp + C + seed)
    x = torch.randn(C, H, W, generator=g)
    return x, torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5


# ------------------------------------------------------------------------------------------------ guarded buffers

TAIL = 384
NAN = float("nan")


def guarded(n, device, tail=TAIL):
    """fp32 [n + tail]: the first n floats NaN (the kernel's output: every element must be written), then a sentinel tail
    (distinct finite values: nothing may be written there)"""
    buf = torch.full((n + tail,), NAN, device=device)
    buf[n:] = _tail_values(tail, device)
    return buf


def _tail_values(tail, device):
    return -(torch.arange(tail, device=device, dtype=torch.float32) + 1000.0)


def tail_intact(buf, n):
    return bool(torch.equal(buf[n:], _tail_values(buf.numel() - n, buf.device)))


def unembed_locator(H):
    """(row, col) of the [C * H, W] view of an image -> channel, image row, token row, token column"""
    def locate(r, c, _=None):
        row = r % H
        seam = f", seam of token rows {row // SH - 1} and {row // SH}" if row % SH == 0 and 0 < row < H - 1 else ""
        return f"channel {r // H}, image row {row} (token row {min(row // SH, (H - KH) // SH)}{seam}), token column {c // KW}"
    return locate
