"""The form rule of the split-f16 GEMM (cra5_gemm_split_form, no GPU): the query against a restatement of the rule as
the launcher had it before the query existed - gemm_dispatch()'s ladder and cra5_gemm_nt_split()'s chunk loop, written
out below -, the launcher's refusal of everything the query refuses, and VAEformer._unembed_launch against the three
places of the model that used to derive the full decode's un-embed launch on their own."""
import copy
import ctypes
import itertools

import pytest

from cra5_amd import _lib, ops, synth
from cra5_amd.vaeformer import VAEformer

GELU, HI, A_PL, W_PL, O_PL, WIDE = 2, 8, 16, 32, 64, 128
PLAIN_ANY = A_PL | W_PL | O_PL
MODE_BITS = (HI, A_PL, W_PL, O_PL, WIDE)


def old_dispatch(M, N, Kp, flags):
    """gemm_dispatch() of one launch (a whole call or one chunk) -> (tile rows, k-step) or None: CRA5_ERR_ARG."""
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128)
    longk, hi, force_wide = Kp > 8192, bool(flags & HI), bool(flags & WIDE)
    if force_wide and (not hi or longk or Kp % 64):
        return None
    if flags & PLAIN_ANY and (not hi or longk or (tiles128 < 256 and not force_wide) or Kp % 64):
        return None
    if longk:
        return 128, 32
    if hi:
        if tiles128 < 256 and not force_wide:
            return 64, 32
        return (256 if M >= 1024 and N >= 2048 else 192), (64 if Kp % 64 == 0 else 32)
    if tiles128 < 256:
        return 64, 32
    if M >= 1024 and N >= 2048:
        return 256, 32
    return (192 if M >= 1024 and N >= 512 else 128), 32


def old_call(M, N, Kp, flags, f32_out, split_out):
    """cra5_gemm_nt_split() -> None (CRA5_ERR_ARG, from the argument checks or from any chunk) or (tile, the set of
    k-steps its launches take, chained, the flags of every launch after the first)."""
    if not (f32_out or split_out) or Kp % 32:
        return None
    if not (Kp > 8192 and f32_out and not split_out and not flags & GELU):
        d = old_dispatch(M, N, Kp, flags)
        return d and (d[0], {d[1]}, False, None)
    nchunk = (Kp + 8191) // 8192
    gran = 64 if (flags & HI and Kp % 64 == 0) else 32
    per = ((Kp // gran + nchunk - 1) // nchunk) * gran
    later = 4 | (flags & (HI | A_PL | W_PL))                       # CRA5_EPI_RES + what the loop carried over
    ds = [old_dispatch(M, N, min(per, Kp - k0), flags if k0 == 0 else later) for k0 in range(0, Kp, per)]
    if any(d is None for d in ds):
        return None
    assert flags & WIDE or len({d[0] for d in ds}) == 1           # (the tile depends on M, N and the WIDE bit alone)
    return ds[0][0], {d[1] for d in ds}, True, later


# M, N on both sides of every threshold: 255 / 256 128 x 128 tiles (15 x 17, 16 x 16, 8 x 31, 8 x 32), M 1023 / 1024,
# N 511 / 512 / 2047 / 2048; the thin model's launches (D = 128, 8 channels: N = 880 columns of the un-embed)
MS = (1, 128, 1023, 1024, 1920, 2048, 10368)
NS = (1, 128, 256, 384, 511, 512, 880, 2047, 2048, 2176, 3968, 4096)
KPS = (32, 64, 96, 8192, 8224, 29504)
# the launches of model 268, (M, N, K), and of the thin model
PRODUCTION = [(10368, n, k) for n, k in ((1024, 29480), (3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (29480, 1024),
                                        (256, 2048), (1024, 256))]
THIN = [(10368, n, k) for n, k in ((128, 880), (384, 128), (128, 128), (512, 128), (128, 512), (880, 128), (32, 256), (128, 32))]


def shapes():
    s = set(itertools.product(MS, NS, KPS))
    s |= {(M, N, (K + 31) // 32 * 32) for M, N, K in PRODUCTION + THIN}
    return sorted(s)


def launcher_status(L, M, N, Kp, flags, f32_out, split_out):
    """cra5_gemm_nt_split on fake pointers (16-byte aligned, never dereferenced: only refused calls are made)."""
    a, w, c, cs, v = (ctypes.c_void_p(i << 24) for i in range(1, 6))
    return L.cra5_gemm_nt_split(a, Kp, w, Kp, c if f32_out else None, N, cs if split_out else None, (N + 31) // 32 * 32,
                                v, v, N, M, N, Kp, 1.0, flags, None)


def test_query_is_the_old_rule_and_the_launcher_refuses_what_it_refuses():
    L = _lib.lib()
    n_ok = n_refused = n_wide_chained = n_mixed = n_hi_longk = 0
    for M, N, Kp in shapes():
        for bits in itertools.product((0, 1), repeat=len(MODE_BITS)):
            mode = sum(b for b, on in zip(MODE_BITS, bits) if on)
            for gelu, f32_out, split_out in itertools.product((0, GELU), (0, 1), (0, 1)):
                flags = mode | gelu
                case = (M, N, Kp, flags, f32_out, split_out)
                got = L.cra5_gemm_split_form(*case)
                old = old_call(*case)
                if old is not None and old[2] and flags & WIDE:
                    # THE named change: the old loop honoured CRA5_GEMM_WIDE_K in the first chunk and dropped it in the
                    # others (later flags carry no WIDE bit) - a form no caller can mean.  Now refused.
                    assert not old[3] & WIDE
                    old, n_wide_chained = None, n_wide_chained + 1
                if old is not None and not old[2] and flags & HI and Kp > 8192:
                    # THE third change: the old ladder sent every one-launch Kp > 8192 (a split output or a GELU) to the
                    # three-product long-K kernel whatever the mode word said - both lo planes read, hi.lo + lo.hi summed,
                    # the lo halves of C_split written.  The reduced-precision mode has no such kernel: now refused.
                    assert old[:2] == (128, {32}) and (split_out or gelu), case
                    old, n_hi_longk = None, n_hi_longk + 1
                if old is None:
                    assert got == ops.ERR_ARG, case
                    assert launcher_status(L, *case) == ops.ERR_ARG, case
                    n_refused += 1
                    continue
                tile, ksteps, chained, _ = old
                if len(ksteps) == 2:
                    # reduced precision, chained, Kp % 64 != 0: the old loop stepped by 64 in whichever chunks happened to be
                    # multiples of 64 and by 32 in the others; one call has one form now, the one every chunk can take
                    assert chained and flags & HI and Kp % 64 and not flags & PLAIN_ANY, case
                    ksteps, n_mixed = {32}, n_mixed + 1
                want = tile | (ops.FORM_K64 if ksteps == {64} else 0) | (ops.FORM_CHAINED if chained else 0) \
                    | (ops.FORM_PLAIN if flags & PLAIN_ANY else 0)
                assert got == want, (case, got, want)
                assert got & ops.FORM_TILE in (64, 128, 192, 256)
                n_ok += 1
    # the sweep saw every kind of answer
    assert n_ok > 1000 and n_refused > 1000 and n_wide_chained > 0 and n_mixed > 0 and n_hi_longk > 0


def test_production_launches_keep_their_forms():
    """Model 268's launches by shape, both precisions: tile and k-step as measured and documented."""
    form = ops.gemm_form
    K64, CH, PL = ops.FORM_K64, ops.FORM_CHAINED, ops.FORM_PLAIN
    M = 10368
    assert form(M, 1024, 29504) == 192 | CH and form(M, 1024, 29504, HI | A_PL | W_PL) == 192 | CH | K64 | PL
    assert form(M, 3072, 1024, 0, False, True) == 256 and form(M, 3072, 1024, HI | A_PL | W_PL | O_PL, False, True) == 256 | K64 | PL
    assert form(M, 1024, 1024) == 192 and form(M, 1024, 4096, HI | A_PL | W_PL) == 192 | K64 | PL
    assert form(M, 4096, 1024, GELU, False, True) == 256
    assert form(M, 29480, 1024) == 256 and form(M, 29480, 1024, HI | W_PL) == 256 | K64 | PL
    assert form(M, 256, 2048) == 64 and form(M, 1024, 256) == 192 and form(M, 256, 2048, HI) == 64
    # a slice of the un-embed names the full launch's k-step; without the word a small problem steps by 32
    assert form(256, 110, 1024, HI | WIDE) == 192 | K64 and form(256, 110, 1024, HI) == 64
    # memoised per argument tuple, and plain_ok is the query
    assert ops.plain_ok(M, 1024, 1024) and not ops.plain_ok(M, 1024, 96) and not ops.plain_ok(1920, 2176, 64)
    assert ops.plain_ok(2048, 2048, 64) and ops.plain_ok(M, 1024, 29504)
    hits = ops.plain_ok.cache_info().hits, ops.gemm_form.cache_info().hits
    assert ops.plain_ok(M, 1024, 1024) and form(M, 1024, 1024) == 192
    assert (ops.plain_ok.cache_info().hits, ops.gemm_form.cache_info().hits) == (hits[0] + 1, hits[1] + 1)


# ---- the model's one helper against the three places that used to decide -----------------------------------------------


def small_model_kwargs():
    """The thin model on an 81 x 160 image: 8 x 16 tokens, so the full un-embed launch (128 x 880) has 7 tiles < 256."""
    kw = copy.deepcopy(synth.thin_model_kwargs())
    kw["ddconfig"]["kwargs"]["img_size"] = (81, 160)
    kw["priorconfig"]["kwargs"]["img_size"] = (8, 16)
    return kw


@pytest.fixture(scope="module", params=["thin", "small"])
def model(request):
    return VAEformer(0, **(synth.thin_model_kwargs() if request.param == "thin" else small_model_kwargs()))


def old_sites(m):
    """-> (weight kind, hi, wide, LayerNorm plain) as _decode_frame / _unembed / _unembed_thinned derived them."""
    cfg = m.cfg
    D, C, (H, W), (kh, kw), (sh, sw) = cfg["embed_dim"], cfg["out_chans"], cfg["img_size"], cfg["patch_size"], cfg["patch_stride"]
    Kp, Mf, Nf = (D + 31) // 32 * 32, m.Hp * m.Wp, C * kh * kw
    hi = m.precision == "f16"
    plain_ok = ((Mf + 127) // 128) * ((Nf + 127) // 128) >= 256 and Kp % 64 == 0                  # ops.plain_ok
    side = (kh, kw, sh, sw) == (11, 10, 10, 10) and H >= kh and W >= kw and (H - kh) % sh == 0 and (W - kw) % sw == 0
    fused = m.gemm_mode == "split" and m.fused_unembed and D <= 8192 and side                    # _fused_unembed_form()[0]
    ln_plain = fused and hi and m.f16_layout == "plain" and D % 64 == 0                            # _fused_unembed_form()[1]
    if fused:      # h.plain is the LayerNorm's; _unembed_thinned: hi and wsp.Kp % 64 == 0
        return ("plain" if ln_plain else "split"), hi, hi and Kp % 64 == 0, ln_plain
    plain_gemm = hi and m.f16_layout == "plain" and m.gemm_mode == "split" and plain_ok          # _plain_gemm
    return ("plain" if plain_gemm else "split"), hi, hi and plain_ok, ln_plain


@pytest.mark.parametrize("precision", ["fp32", "f16"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("layout", ["plain", "split"])
def test_unembed_launch_is_what_the_three_sites_derived(model, precision, fused, layout):
    model.precision, model.fused_unembed, model.f16_layout = precision, fused, layout
    big = ((model.Hp * model.Wp + 127) // 128) * 7 >= 256
    assert big == (model.cfg["img_size"] == (721, 1440))
    assert model._unembed_launch() == old_sites(model)
    kind, hi, wide, a_plain = model._unembed_launch()
    assert hi == (precision == "f16") and wide == (hi and (fused or big))
    assert (kind == "plain") == (wide and layout == "plain") and a_plain == (fused and kind == "plain")
    model.gemm_mode = "f32"
    try:
        assert model._unembed_launch() == ("f32", False, False, False)
    finally:
        model.gemm_mode = "split"
