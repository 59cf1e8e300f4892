"""The device kernels that decide the stream's integers - gaussian_conditional_kernel, gaussian_conditional_compact_kernel,
resolve_symbols_kernel<WideRecords / CompactRecords>, entropy_bottleneck_kernel (csrc/elementwise.hip, csrc/rans_resolve.h)
- against the numpy references of tests/entropy_helpers.py on its input domains: exact rounding ties and their float32
neighbours, -0.0 residuals, residuals beyond 2^23, every scale-table entry and its neighbours, the lower bound from both
sides, every table row with every escape payload at a nibble edge, invalid rows, launches whose grid-stride loop takes a
second, ragged trip.

Every comparison is array_equal on integers, or on the uint32 view of y_hat / z_hat; no element is left out and nothing
is allowed to flip.  A failure names the first differing position, its class and its inputs.  (The likelihoods are
floating point and are held elsewhere: test_kernels_gpu.py, test_model_gpu.py.)"""
import time

import numpy as np
import pytest
import torch

import entropy_helpers as E
from cra5_amd import ops
from cra5_amd._lib import Cra5Error, ERR_RANGE

pytestmark = pytest.mark.gpu

GRID_THREADS = 1048576             # grid_for(): 4096 blocks x 256 threads; beyond it a launch grid-strides
BIG = GRID_THREADS + 257           # the smallest size whose second trip is ragged
SIZES = (1, 255, 256, 257, BIG)
ERR_ARG = -7
CANARY = 0xA5


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # (a copy: the domains are read-only)


def _np(t):
    return t.cpu().numpy()


class _Tally:
    def __init__(self, what):
        self.what, self.n, self.t0 = what, 0, time.perf_counter()

    def add(self, n):
        self.n += n

    def done(self):
        print(f"{self.what}: {self.n} elements compared, all equal, {time.perf_counter() - self.t0:.2f} s")


# ------------------------------------------------------------------------------------------------ gaussian_conditional

@pytest.fixture(scope="module")
def gc_big():
    """the residual and the scale domain (production table), each repeated to BIG elements, with gc_ref's answer: computed
    once, read-only; a smaller launch takes a prefix"""
    table = E.production_table()
    y, mu, rc = E.fill(BIG, *E.residual_domain())
    s, sc = E.fill(BIG, *E.scale_domain(table), phase=5)
    idx, sym, y_hat = E.gc_ref(s, mu, table, y=y)
    assert E.residual_domain()[0].size <= BIG and int(np.abs(sym).max()) < 2 ** 31
    out = dict(table=table, y=y, mu=mu, s=s, rc=rc, sc=sc, idx=idx, sym=sym, y_hat=y_hat)
    for a in out.values():
        a.setflags(write=False)
    return out


WANTS = [("idx",), ("sym",), ("y_hat",), ("idx", "sym"), ("idx", "y_hat"), ("sym", "y_hat"), ("idx", "sym", "y_hat")]


@pytest.mark.parametrize("n", SIZES)
def test_gaussian_conditional_integers(dev, gc_big, n):
    g = {k: (v[:n] if k != "table" else v) for k, v in gc_big.items()}
    tally = _Tally(f"gaussian_conditional_kernel, n = {n}")
    table, y, mu, s = (_t(g[k], dev) for k in ("table", "y", "mu", "s"))
    res_in, sc_in = dict(y=g["y"], mu=g["mu"]), dict(scale=g["s"])
    for want in WANTS:
        o = ops.gaussian_conditional(s, mu, table, y=y, want=want)
        assert set(o) == set(want)
        if "idx" in want:
            tally.add(E.compare_ints(_np(o["idx"]), g["idx"], g["sc"], E.SCALE_CLASSES, sc_in, f"idx, want={want}"))
        if "sym" in want:
            tally.add(E.compare_ints(_np(o["sym"]), g["sym"], g["rc"], E.RES_CLASSES, res_in, f"sym, want={want}"))
        if "y_hat" in want:
            tally.add(E.compare_ints(_np(o["y_hat"]), g["y_hat"], g["rc"], E.RES_CLASSES, res_in, f"y_hat, want={want}"))
    # the decode side: the symbols back in; y_hat equal to the y path's (no mean of the domain is -0.0)
    sym_in = _t(g["sym"].astype(np.int32), dev)
    d = ops.gaussian_conditional(s, mu, table, sym_in=sym_in, want=("idx", "sym", "y_hat"))
    ref = E.gc_ref(g["s"], g["mu"], g["table"], sym_in=g["sym"])
    assert np.array_equal(ref[2].view(np.uint32), g["y_hat"].view(np.uint32))
    res_in = dict(sym=g["sym"], mu=g["mu"])
    tally.add(E.compare_ints(_np(d["y_hat"]), g["y_hat"], g["rc"], E.RES_CLASSES, res_in, "y_hat from sym_in"))
    tally.add(E.compare_ints(_np(d["sym"]), g["sym"], g["rc"], E.RES_CLASSES, res_in, "sym from sym_in"))
    tally.add(E.compare_ints(_np(d["idx"]), g["idx"], g["sc"], E.SCALE_CLASSES, sc_in, "idx beside sym_in"))
    tally.done()


def test_gaussian_conditional_signed_zero(dev):
    """q = -0.0 under a mean of -0.0: the y path gives -0.0, the sym_in path +0.0 - each its own reference's bits"""
    y, mu = E.signed_zero_cases()
    table, s = _t(E.production_table(), dev), torch.ones(y.size, device=dev)
    cls = np.full(y.size, E.R_NEGZERO, dtype=np.uint8)
    o = ops.gaussian_conditional(s, _t(mu, dev), table, y=_t(y, dev), want=("sym", "y_hat"))
    _, sym, y_hat = E.gc_ref(None, mu, None, y=y)
    E.compare_ints(_np(o["sym"]), sym, cls, E.RES_CLASSES, dict(y=y, mu=mu), "sym")
    E.compare_ints(_np(o["y_hat"]), y_hat, cls, E.RES_CLASSES, dict(y=y, mu=mu), "y_hat")
    d = ops.gaussian_conditional(s, _t(mu, dev), table, sym_in=o["sym"], want=("y_hat",))
    E.compare_ints(_np(d["y_hat"]), E.gc_ref(None, mu, None, sym_in=sym)[2], cls, E.RES_CLASSES, dict(sym=sym, mu=mu), "y_hat from sym_in")
    c = ops.gaussian_conditional_compact(None, _t(mu, dev), sym16_in=o["sym"].to(torch.int16))
    E.compare_ints(_np(c["y_hat"]), _np(d["y_hat"]), cls, E.RES_CLASSES, dict(sym=sym, mu=mu), "compact y_hat from sym16_in")


TABLE_CASES = [("synthetic", 1, E.BOUND), ("synthetic", 2, E.BOUND), ("synthetic", 255, E.BOUND), ("synthetic", 256, E.BOUND),
               ("production", 64, E.INNER_BOUND)]


@pytest.mark.parametrize("kind,n_table,bound", TABLE_CASES)
def test_scale_index_on_other_tables_and_bounds(dev, kind, n_table, bound):
    """n_table in {1, 2, 255, 256} (256 must reach row 255, also through the uint8 store), and the production table under
    a bound that lies inside it - the only place where a dropped LowerBound changes a row"""
    table = E.synthetic_table(n_table) if kind == "synthetic" else E.production_table()
    s, sc = E.scale_domain(table, bound)
    want = E.scale_index_ref(s, table, bound)
    lowest = int(E.scale_index_ref([0.0], table, bound)[0])           # the row of the bound itself
    assert int(want.max()) == n_table - 1 and int(want.min()) == lowest and (lowest > 0) == (bound == E.INNER_BOUND)
    tally = _Tally(f"scale index, {kind} table of {n_table}, bound {bound}")
    mu = torch.zeros(s.size, device=dev)
    o = ops.gaussian_conditional(_t(s, dev), mu, _t(table, dev), sym_in=torch.zeros(s.size, device=dev, dtype=torch.int32),
                                 want=("idx",), scale_bound=bound)
    tally.add(E.compare_ints(_np(o["idx"]), want, sc, E.SCALE_CLASSES, dict(scale=s), "idx"))
    c = ops.gaussian_conditional_compact(_t(s, dev), mu, _t(table, dev), want_idx8=True, scale_bound=bound)
    assert c["idx8"].dtype == torch.uint8
    tally.add(E.compare_ints(_np(c["idx8"]), want, sc, E.SCALE_CLASSES, dict(scale=s), "idx8"))
    tally.done()


def test_a_table_of_257_entries_is_refused(dev):
    table = _t(np.geomspace(E.BOUND, 256.0, 257).astype(np.float32), dev)
    s, mu = torch.ones(300, device=dev), torch.zeros(300, device=dev)
    with pytest.raises(Cra5Error) as ei:
        ops.gaussian_conditional(s, mu, table, y=s, want=("idx", "sym"))
    assert ei.value.status == ERR_ARG
    with pytest.raises(Cra5Error) as ei:
        ops.gaussian_conditional_compact(s, mu, table, want_idx8=True)
    assert ei.value.status == ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the compact kernel

def test_compact_indexes_match_the_int32_kernel(dev, gc_big):
    g = gc_big
    tally = _Tally("gaussian_conditional_compact_kernel, idx8")
    table, s, mu = _t(g["table"], dev), _t(g["s"], dev), _t(g["mu"], dev)
    c = ops.gaussian_conditional_compact(s, mu, table, want_idx8=True)
    tally.add(E.compare_ints(_np(c["idx8"]), g["idx"], g["sc"], E.SCALE_CLASSES, dict(scale=g["s"]), "idx8"))
    o = ops.gaussian_conditional(s, mu, table, sym_in=torch.zeros(BIG, device=dev, dtype=torch.int32), want=("idx",))
    assert torch.equal(c["idx8"].to(torch.int32), o["idx"])
    # idx8_out= a slice at an odd byte offset inside a larger buffer: the bytes on both sides stay
    for n in (257, 4301, BIG):
        buf = torch.full((13 + n + 64,), CANARY, device=dev, dtype=torch.uint8)
        r = ops.gaussian_conditional_compact(s[:n], mu[:n], table, want_idx8=True, idx8_out=buf[13:13 + n])
        assert r["idx8"].data_ptr() == buf.data_ptr() + 13
        b = _np(buf)
        assert bool((b[:13] == CANARY).all()) and bool((b[13 + n:] == CANARY).all()), n
        tally.add(E.compare_ints(b[13:13 + n], g["idx"][:n], g["sc"][:n], E.SCALE_CLASSES, dict(scale=g["s"][:n]), f"idx8_out, n = {n}"))
    tally.done()


def test_compact_y_hat_for_every_int16(dev):
    means = np.array([0.0, -0.0, 0.1, 63.999, -1.0 / 3.0], dtype=np.float32)
    assert means.view(np.uint32)[2] & 1 and np.signbit(means[1])          # (0.1f = 0x3dcccccd: an odd mantissa)
    sym = np.tile(np.arange(-32768, 32768, dtype=np.int64), means.size)
    mu = np.repeat(means, 65536)
    _, _, want = E.gc_ref(None, mu, None, sym_in=sym)
    cls = np.zeros(sym.size, dtype=np.uint8)
    tally = _Tally("gaussian_conditional_compact_kernel, y_hat from sym16_in")
    c = ops.gaussian_conditional_compact(None, _t(mu, dev), sym16_in=_t(sym.astype(np.int16), dev))
    tally.add(E.compare_ints(_np(c["y_hat"]), want, cls, E.RES_CLASSES, dict(sym=sym, mu=mu), "y_hat"))
    o = ops.gaussian_conditional(torch.ones(sym.size, device=dev), _t(mu, dev), None, sym_in=_t(sym.astype(np.int32), dev),
                                 want=("y_hat",))
    tally.add(E.compare_ints(_np(o["y_hat"]), want, cls, E.RES_CLASSES, dict(sym=sym, mu=mu), "int32 kernel's y_hat"))
    assert torch.equal(c["y_hat"].view(torch.int32), o["y_hat"].view(torch.int32))
    tally.done()


# ------------------------------------------------------------------------------------------------ resolve

def _dev_tables(tables, dev):
    return tuple(_t(a, dev) for a in tables)


@pytest.mark.parametrize("which", ["production", "ragged"])
def test_resolve_records_match_the_reference(dev, which):
    sym, idx, cls, tables = E.resolve_domain(which)
    cdf, lens, offs = tables
    ins = dict(sym=sym, idx=idx)
    sr_w, raw_w, esc_w, rec_w, ovf_w = E.resolve_ref(sym, idx, cdf, lens, offs)
    tally = _Tally(f"resolve_symbols_kernel, {which} tables")
    dt = _dev_tables(tables, dev)
    sr, raw, esc = ops.rans_resolve_symbols(_t(sym, dev), _t(idx, dev), *dt)
    sr2, rec, ovf = ops.rans_resolve_symbols_compact(_t(sym, dev), _t(idx, dev), *dt)
    sr, raw, esc = _np(sr).view(np.uint32), _np(raw).view(np.uint32), _np(esc)
    sr2, rec = _np(sr2).view(np.uint32), _np(rec).view(np.uint16)
    for got, want, label in ((sr, sr_w, "sr"), (raw, raw_w, "raw"), (esc, esc_w, "esc"), (sr2, sr_w, "compact sr"),
                             (rec, rec_w, "rec16")):
        tally.add(E.compare_ints(got, want, cls, E.RESOLVE_CLASSES, ins, label))
    assert int(ovf[0]) == ovf_w == 1
    narrow = rec != 0xFFFF
    assert np.array_equal(rec[narrow] >> 12, esc[narrow]) and np.array_equal(rec[narrow] & 0xFFF, raw[narrow])
    bad = (cls & E.V_INVALID) != 0
    assert bool((esc[bad] == 255).all()) and bool((rec[bad] == 0xFFFF).all()) and not sr[bad].any() and not raw[bad].any()
    # the device's records through the host coder, on the part a stream can hold
    keep = E.codable(cls)
    s, i = sym[keep], idx[keep]
    stream = ops.rans_encode(s, i, cdf, lens, offs)
    assert ops.rans_encode_resolved(sr[keep], raw[keep], esc[keep]) == stream
    assert np.array_equal(ops.rans_decode(stream, i, cdf, lens, offs), s)
    with pytest.raises(Cra5Error) as ei:
        ops.rans_encode_resolved_compact(sr2[keep], rec[keep])
    assert ei.value.status == ERR_RANGE
    fit = keep & narrow
    s, i = sym[fit], idx[fit]
    sr3, rec3, ovf3 = ops.rans_resolve_symbols_compact(_t(s, dev), _t(i, dev), *dt)
    assert int(ovf3[0]) == 0
    tally.add(E.compare_ints(_np(rec3).view(np.uint16), rec_w[fit], cls[fit], E.RESOLVE_CLASSES, dict(sym=s, idx=i), "rec16, narrow part"))
    stream = ops.rans_encode(s, i, cdf, lens, offs)
    assert ops.rans_encode_resolved_compact(_np(sr3), _np(rec3)) == stream
    assert np.array_equal(ops.rans_decode(stream, i, cdf, lens, offs), s)
    tally.done()


def test_resolve_overflow_word(dev):
    """0 on a launch without a wide escape or an invalid row, whatever the word held before; 1 when exactly one element is
    wide or invalid - the first, the last, one inside the second grid-stride trip - and every other record still right"""
    sym_d, idx_d, cls_d, tables = E.resolve_domain("production")
    cdf, lens, offs = tables
    calm = (cls_d & (E.V_WIDE | E.V_INVALID)) == 0
    sym, idx, cls = E.fill(BIG, sym_d[calm], idx_d[calm], cls_d[calm])
    sr_w, _, _, rec_w, ovf_w = E.resolve_ref(sym, idx, cdf, lens, offs)
    assert ovf_w == 0 and bool((cls & E.V_ESCAPE).any())
    tally = _Tally("resolve_symbols_kernel<CompactRecords>, overflow word")
    dt = _dev_tables(tables, dev)
    sym_t, idx_t = _t(sym, dev), _t(idx, dev)
    out = (torch.empty(BIG, device=dev, dtype=torch.int32), torch.empty(BIG, device=dev, dtype=torch.int16),
           torch.ones(1, device=dev, dtype=torch.int32))

    def launch(label, sym_t, idx_t, sr_want, rec_want, ovf_want, s_np, i_np):
        out[2].fill_(1 - ovf_want)                                   # the word holds the other answer before the call
        sr, rec, ovf = ops.rans_resolve_symbols_compact(sym_t, idx_t, *dt, out=out)
        assert int(ovf[0]) == ovf_want, label
        ins = dict(sym=s_np, idx=i_np)
        tally.add(E.compare_ints(_np(sr).view(np.uint32), sr_want, cls, E.RESOLVE_CLASSES, ins, f"sr, {label}"))
        tally.add(E.compare_ints(_np(rec).view(np.uint16), rec_want, cls, E.RESOLVE_CLASSES, ins, f"rec16, {label}"))

    launch("calm", sym_t, idx_t, sr_w, rec_w, 0, sym, idx)
    row = 20
    wide_sym = int(offs[row]) + int(lens[row]) - 2 + 2048            # payload 4096: the first that does not fit
    for pos, (s1, i1) in ((0, (wide_sym, row)), (BIG - 1, (0, -1)), (GRID_THREADS + 100, (wide_sym, row)), (0, (5, cdf.shape[0])),
                          (BIG - 1, (wide_sym, row)), (GRID_THREADS + 100, (0, E.INT32_MAX))):
        s2, i2 = sym_t.clone(), idx_t.clone()
        s2[pos], i2[pos] = s1, i1
        s_np, i_np, sr_1, rec_1 = sym.copy(), idx.copy(), sr_w.copy(), rec_w.copy()
        s_np[pos], i_np[pos] = s1, i1
        one = E.resolve_ref([s1], [i1], cdf, lens, offs)
        sr_1[pos], rec_1[pos] = one[0][0], one[3][0]
        assert rec_1[pos] == 0xFFFF and one[4] == 1
        launch(f"one {'invalid row' if i1 != row else 'wide escape'} at {pos}", s2, i2, sr_1, rec_1, 1, s_np, i_np)
    tally.done()


def test_resolve_into_slices_of_a_packed_buffer(dev):
    """out= as slices of one canary-filled buffer: rec16 at a 2-byte-aligned, not 4-byte-aligned offset, esc at an odd
    offset; the bytes between and around the records stay"""
    sym, idx, cls, tables = E.resolve_domain("ragged")
    cdf, lens, offs = tables
    n = sym.size
    sr_w, raw_w, esc_w, rec_w, _ = E.resolve_ref(sym, idx, cdf, lens, offs)
    dt = _dev_tables(tables, dev)
    ins = dict(sym=sym, idx=idx)

    def packed(parts):
        """[(name, offset, bytes)] -> a canary buffer and what lies outside the parts"""
        total = max(o + b for _, o, b in parts) + 32
        buf = torch.full((total,), CANARY, device=dev, dtype=torch.uint8)
        free = np.ones(total, dtype=bool)
        for _, o, b in parts:
            assert not (~free[o:o + b]).any()
            free[o:o + b] = False
        return buf, free

    # wide records: sr, raw int32, esc uint8 at an odd offset
    o_sr, o_raw, o_esc = 16, 16 + 4 * n + 8, 16 + 8 * n + 8 + 8 + 3
    assert o_esc % 2 == 1 and o_raw % 4 == 0
    buf, free = packed([("sr", o_sr, 4 * n), ("raw", o_raw, 4 * n), ("esc", o_esc, n)])
    out = (buf[o_sr:o_sr + 4 * n].view(torch.int32), buf[o_raw:o_raw + 4 * n].view(torch.int32), buf[o_esc:o_esc + n])
    ops.rans_resolve_symbols(_t(sym, dev), _t(idx, dev), *dt, out=out)
    b = _np(buf)
    assert bool((b[free] == CANARY).all()) and int(free.sum()) == 16 + 8 + 11 + 32
    E.compare_ints(b[o_sr:o_sr + 4 * n].view(np.uint32), sr_w, cls, E.RESOLVE_CLASSES, ins, "packed sr")
    E.compare_ints(b[o_raw:o_raw + 4 * n].view(np.uint32), raw_w, cls, E.RESOLVE_CLASSES, ins, "packed raw")
    E.compare_ints(b[o_esc:o_esc + n], esc_w, cls, E.RESOLVE_CLASSES, ins, "packed esc")
    # compact records: rec16 at 2 (mod 4)
    o_rec = 16 + 4 * n + 6
    o_ovf = (o_rec + 2 * n + 8 + 3) // 4 * 4
    assert o_rec % 4 == 2
    buf, free = packed([("sr", o_sr, 4 * n), ("rec", o_rec, 2 * n), ("ovf", o_ovf, 4)])
    out = (buf[o_sr:o_sr + 4 * n].view(torch.int32), buf[o_rec:o_rec + 2 * n].view(torch.int16), buf[o_ovf:o_ovf + 4].view(torch.int32))
    ops.rans_resolve_symbols_compact(_t(sym, dev), _t(idx, dev), *dt, out=out)
    b = _np(buf)
    assert bool((b[free] == CANARY).all())
    E.compare_ints(b[o_sr:o_sr + 4 * n].view(np.uint32), sr_w, cls, E.RESOLVE_CLASSES, ins, "packed compact sr")
    E.compare_ints(b[o_rec:o_rec + 2 * n].view(np.uint16), rec_w, cls, E.RESOLVE_CLASSES, ins, "packed rec16")
    assert int(b[o_ovf:o_ovf + 4].view(np.int32)[0]) == 1
    print(f"resolve_symbols_kernel into packed slices: {5 * n} records and {2 * int(free.sum())} canary bytes compared, all equal")


# ------------------------------------------------------------------------------------------------ entropy_bottleneck

@pytest.mark.parametrize("C,n_per_ch", E.EB_SHAPES)
def test_entropy_bottleneck_integers(dev, C, n_per_ch):
    z, med, cls = E.eb_domain(C, n_per_ch)
    sym_w, z_hat_w = E.eb_ref(med, n_per_ch, z=z)
    ch = np.repeat(np.arange(C), n_per_ch)
    ins = dict(z=z, channel=ch, median=np.repeat(med, n_per_ch))
    tally = _Tally(f"entropy_bottleneck_kernel, {C} x {n_per_ch}")
    med_t = _t(med, dev)
    for want in (("sym", "z_hat"), ("sym",), ("z_hat",)):
        o = ops.entropy_bottleneck(med_t, None, z=_t(z, dev), want=want)
        assert set(o) == set(want)
        if "sym" in want:
            assert o["sym"].shape == (C, n_per_ch)
            tally.add(E.compare_ints(_np(o["sym"]), sym_w, cls, E.RES_CLASSES, ins, f"sym, want={want}"))
        if "z_hat" in want:
            tally.add(E.compare_ints(_np(o["z_hat"]), z_hat_w, cls, E.RES_CLASSES, ins, f"z_hat, want={want}"))
    sym_in = _t(sym_w.astype(np.int32).reshape(C, n_per_ch), dev)
    d = ops.entropy_bottleneck(med_t, None, sym_in=sym_in, want=("sym", "z_hat"))
    ref = E.eb_ref(med, n_per_ch, sym_in=sym_w)
    assert np.array_equal(ref[1].view(np.uint32), z_hat_w.view(np.uint32))
    ins = dict(sym=sym_w, channel=ch, median=ins["median"])
    tally.add(E.compare_ints(_np(d["z_hat"]), z_hat_w, cls, E.RES_CLASSES, ins, "z_hat from sym_in"))
    tally.add(E.compare_ints(_np(d["sym"]), sym_w, cls, E.RES_CLASSES, ins, "sym from sym_in"))
    tally.done()
