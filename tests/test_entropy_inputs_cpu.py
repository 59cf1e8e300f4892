"""The integer references and input domains of tests/entropy_helpers.py, checked without a GPU: every class of every
domain is populated, the references agree with what the project already trusts (oracle/torch_ref.py for the float ->
integer decisions, the host coder for the resolved records), and one deliberately wrong reference per fault the GPU
tests are meant to catch differs from the true one somewhere on the domain - the class that catches it is printed."""
import numpy as np
import pytest
import torch

import entropy_helpers as E
from cra5_amd import ops
from cra5_amd._lib import Cra5Error, ERR_RANGE
from oracle import torch_ref as R


def _counts(cls, names):
    return ", ".join(f"{n} {int(((np.asarray(cls) >> i) & 1).sum())}" for i, n in enumerate(names))


def _populated(cls, names, label):
    print(f"{label}: {np.asarray(cls).size} elements; per class: {_counts(cls, names)}")
    for i, n in enumerate(names):
        assert int(((np.asarray(cls) >> i) & 1).sum()) > 0, (label, n)


TABLES = [("production", E.production_table)] + [(f"synthetic {n}", (lambda n=n: E.synthetic_table(n))) for n in (1, 2, 255, 256)]


# ------------------------------------------------------------------------------------------------ populated

def test_residual_domain_holds_every_class():
    y, mu, c = E.residual_domain()
    _populated(c, E.RES_CLASSES, "residual domain")
    assert y.dtype == mu.dtype == np.float32 and not y.flags.writeable and y.size < 2 ** 20
    q = np.rint(y - mu)
    assert bool(np.isfinite(y).all()) and float(np.abs(q).max()) < 2.0 ** 31
    # every integer k in [-300, 300] is a tie of every mean; rint sends them to even
    tie = (c & E.R_TIE) != 0
    for m in E.tie_means():
        k = np.unique(np.floor((y - mu)[tie & (mu == m)]))
        assert np.array_equal(k, np.arange(-300, 301)), float(m)
    assert bool((q[tie] % 2 == 0).all())
    assert bool((np.abs(mu[c != E.R_RANDOM] * 1024) % 1 == 0).all()) and float(np.abs(mu[c != E.R_RANDOM]).max()) < 64
    big = np.abs((y - mu)[(c & E.R_LARGE) != 0]).astype(np.float64)
    assert {float(np.float32(v)) for v in E.LARGE} <= set(np.unique(big).tolist())      # (each exactly, under the mean 0)


@pytest.mark.parametrize("name,make", TABLES, ids=[t[0] for t in TABLES])
def test_scale_domain_holds_every_class(name, make):
    table = make()
    s, c = E.scale_domain(table)
    _populated(c, E.SCALE_CLASSES, f"scale domain, {name} table")
    for t in table:
        for v in (t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))):
            assert bool((s == v).any())
    for v in (np.float32(E.BOUND), np.float32(0), np.finfo(np.float32).smallest_subnormal, E.FLT_MAX):
        assert bool((s == v).any())
    assert bool(np.signbit(s[s == 0]).any()) and bool((s < 0).any())
    idx = E.scale_index_ref(s, table)
    assert set(np.unique(idx)) == set(range(table.size)), "every row of the table is reached"


@pytest.mark.parametrize("which", ["production", "ragged"])
def test_resolve_domain_holds_every_class(which):
    sym, idx, c, (cdf, lens, offs) = E.resolve_domain(which)
    names = E.RESOLVE_CLASSES if which == "ragged" else E.RESOLVE_CLASSES[:-1]
    _populated(c, names, f"resolve domain, {which} tables")
    assert sym.dtype == idx.dtype == np.int32 and sym.size < 2 ** 20
    sr, raw, esc, rec, overflow = E.resolve_ref(sym, idx, cdf, lens, offs)
    assert overflow == 1
    ok = E.row_valid(idx, cdf, lens)
    for r in range(cdf.shape[0]):
        here = ok & (idx == r)
        if not 2 <= lens[r] <= cdf.shape[1]:
            assert not here.any() and bool(((idx == r) & ((c & E.V_INVALID) != 0)).any())
            continue
        # every symbol from offset - 40 to offset + length + 40, and every payload from its own side
        assert set(range(offs[r] - 40, offs[r] + lens[r] + 41)) <= set(sym[here].tolist())
        below, above = here & (sym < offs[r]), here & (sym >= offs[r])
        want = [p for p in E.PAYLOADS if (p % 2 or lens[r] == 2 or p < 2 ** 31 - 2)]
        assert set(p for p in want if p % 2) <= set(raw[below].tolist()), r
        assert set(p for p in want if not p % 2) <= set(raw[above & (esc > 0)].tolist()), r
    for bad in (-1, cdf.shape[0], E.INT32_MAX):
        assert bool((idx == bad).any())
    if which == "ragged":
        assert 3 in lens and cdf.shape[1] in lens and 1 in lens and cdf.shape[1] + 1 in lens
        assert bool((offs > 0).any()) and bool((offs == 0).any()) and bool((offs < 0).any())
    v = sym.astype(np.int64)[ok] - offs.astype(np.int64)[idx[ok]]
    assert int(np.abs(v).max()) == E.V_LIMIT
    # esc = 1 + nibbles takes every value 1..9; the compact record's edge is met from both sides
    assert set(np.unique(esc)) == set(range(10)) | {255}
    assert bool((rec[raw == 4095] == (0x4000 | 4095)).all()) and bool((rec[raw == 4096] == 0xFFFF).all())
    assert bool((rec[(esc == 1)] == 0x1000).all()) and bool((esc == 1).any())


@pytest.mark.parametrize("C,n", E.EB_SHAPES)
def test_bottleneck_domain_holds_every_class(C, n):
    z, med, c = E.eb_domain(C, n)
    print(f"bottleneck domain {C} x {n}: per class: {_counts(c, E.RES_CLASSES)}")
    assert z.shape == c.shape == (C, n) and np.unique(med).size == C
    if n >= 8:
        for bit in (E.R_TIE, E.R_NEAR, E.R_NEGZERO, E.R_INT, E.R_RANDOM):
            assert bool(((c & bit) != 0).any(axis=1)[0::2].all()), bit       # every channel whose median allows ties
        assert bool(((c[1::2] & E.R_TIE) == 0).all())
    else:
        assert int(c[0, 0]) == E.R_TIE
    if C > 1:
        frac = med.astype(np.float64) * 1024 % 1
        assert bool((frac[0::2] == 0).all()) and bool((frac[1::2] != 0).all())
        assert bool(((med[1::2].view(np.uint32) & 0xFF) != 0).any()), "some medians with full mantissas"


# ------------------------------------------------------------------------------------------------ against the oracle

def test_gc_ref_matches_the_oracle_on_the_residual_domain():
    y, mu, _ = E.residual_domain()
    _, sym, y_hat = E.gc_ref(None, mu, None, y=y)
    ty, tm = torch.from_numpy(y.copy()), torch.from_numpy(mu.copy())
    assert np.array_equal(sym, R.gc_symbols(ty, tm).numpy().astype(np.int64))
    o_hat, _ = R.gc_forward(ty, torch.ones_like(ty), tm)
    assert np.array_equal(y_hat.view(np.uint32), o_hat.numpy().view(np.uint32))
    # the decode side: the symbols back in give y_hat again (no mean of the domain is -0.0)
    _, sym2, y_hat2 = E.gc_ref(None, mu, None, sym_in=sym)
    assert np.array_equal(sym2, sym) and np.array_equal(y_hat2.view(np.uint32), y_hat.view(np.uint32))
    zy, zm = E.signed_zero_cases()
    _, zs, a = E.gc_ref(None, zm, None, y=zy)
    _, _, b = E.gc_ref(None, zm, None, sym_in=zs)
    differ = a.view(np.uint32) != b.view(np.uint32)
    assert differ.tolist() == [True, True, False, False, False, False, False, False, False] and bool((a == b).all())


@pytest.mark.parametrize("name,make", TABLES, ids=[t[0] for t in TABLES])
def test_gc_ref_matches_the_oracle_on_the_scale_domain(name, make):
    table = make()
    s, _ = E.scale_domain(table)
    idx = E.scale_index_ref(s, table)
    want = R.gc_build_indexes(torch.from_numpy(s.copy()), torch.from_numpy(table.copy()), bound=E.BOUND)
    assert np.array_equal(idx, want.numpy().astype(np.int64))
    assert int(idx.min()) == 0 and int(idx.max()) == table.size - 1
    if name == "production":
        assert np.array_equal(table, R.get_scale_table().numpy())


@pytest.mark.parametrize("C,n", E.EB_SHAPES)
def test_eb_ref_matches_the_oracle(C, n):
    z, med, _ = E.eb_domain(C, n)
    sd = {"entropy_bottleneck.quantiles": torch.from_numpy(np.stack([med - 1, med, med + 1], axis=1).reshape(C, 1, 3).copy())}
    sym, z_hat = E.eb_ref(med, n, z=z)
    tz = torch.from_numpy(z.copy()).reshape(1, C, n)
    assert np.array_equal(sym, R.eb_symbols(tz, sd).numpy().reshape(-1).astype(np.int64))
    m = R.eb_medians(sd).reshape(1, C, 1)
    want = torch.round(tz - m) + m                                    # eb_forward's z_hat (torch_ref.py, entropy_models.py:465-510)
    assert np.array_equal(z_hat.view(np.uint32), want.numpy().reshape(-1).view(np.uint32))
    sym2, z_hat2 = E.eb_ref(med, n, sym_in=sym)
    assert np.array_equal(sym2, sym) and np.array_equal(z_hat2.view(np.uint32), z_hat.view(np.uint32))


# ------------------------------------------------------------------------------------------------ against the host coder

@pytest.mark.parametrize("which", ["production", "ragged"])
def test_resolve_ref_matches_the_host_coder(which):
    sym, idx, c, (cdf, lens, offs) = E.resolve_domain(which)
    keep = E.codable(c)
    s, i = sym[keep], idx[keep]
    sr, raw, esc, rec, overflow = E.resolve_ref(s, i, cdf, lens, offs)
    stream = ops.rans_encode(s, i, cdf, lens, offs)
    assert ops.rans_encode_resolved(sr, raw, esc) == stream
    assert np.array_equal(ops.rans_decode(stream, i, cdf, lens, offs), s)
    assert overflow == 1
    with pytest.raises(Cra5Error) as ei:
        ops.rans_encode_resolved_compact(sr, rec)
    assert ei.value.status == ERR_RANGE
    narrow = rec != 0xFFFF
    assert np.array_equal(narrow, raw < 4096)
    sr_n, raw_n, esc_n, rec_n, overflow_n = E.resolve_ref(s[narrow], i[narrow], cdf, lens, offs)
    assert overflow_n == 0 and np.array_equal(rec_n, rec[narrow])
    assert ops.rans_encode_resolved_compact(sr_n, rec_n) == ops.rans_encode(s[narrow], i[narrow], cdf, lens, offs)
    # the invalid rows: records no encoder takes
    bad = (c & E.V_INVALID) != 0
    sr_b, raw_b, esc_b, rec_b, _ = E.resolve_ref(sym[bad], idx[bad], cdf, lens, offs)
    assert not sr_b.any() and not raw_b.any() and bool((esc_b == 255).all()) and bool((rec_b == 0xFFFF).all())
    with pytest.raises(Cra5Error):
        ops.rans_encode_resolved(sr_b, raw_b, esc_b)
    with pytest.raises(Cra5Error):
        ops.rans_encode(sym[bad][:1], idx[bad][:1], cdf, lens, offs)
    if which == "ragged":      # the full-range row resolves to frequency 0, which every encoder refuses
        full = (c & E.V_FULLROW) != 0
        sr_f, raw_f, esc_f, _, _ = E.resolve_ref(sym[full], idx[full], cdf, lens, offs)
        assert not sr_f.any() and bool((esc_f > 0).all())
        with pytest.raises(Cra5Error):
            ops.rans_encode_resolved(sr_f, raw_f, esc_f)


# ------------------------------------------------------------------------------------------------ mutants

def _caught(name, differs, cls, names):
    assert bool(differs.any()), f"mutant '{E.MUTANTS[name]}' equals the reference on the whole domain"
    c = np.asarray(cls).reshape(-1)[differs.reshape(-1)]
    by = {n: int(((c >> i) & 1).sum()) for i, n in enumerate(names)}
    print(f"mutant '{E.MUTANTS[name]}': caught at {int(differs.sum())} elements, by class: "
          + ", ".join(f"{n} {k}" for n, k in by.items() if k))
    return by


def test_every_scale_mutant_is_caught():
    table = E.production_table()
    s, c = E.scale_domain(table)
    true = E.scale_index_ref(s, table)
    lt = E.scale_index_ref(s, table, mutant="search_lt") != true
    by = _caught("search_lt", lt, c, E.SCALE_CLASSES)
    # each entry but the last, and whatever the bound lifts onto entry 0 (the production table starts AT the bound)
    assert by["entry"] == 63 and by["above-entry"] == 0 and bool((((c & E.S_ENTRY) != 0) | (s <= table[0]))[lt].all())
    by = _caught("index_unclamped", E.scale_index_ref(s, table, mutant="index_unclamped") != true, c, E.SCALE_CLASSES)
    assert by["FLT_MAX"] == 1 and by["above-entry"] == 1 and by["entry"] == 0
    # with the table starting at the bound, dropping the bound moves nothing: every scale under it lands in row 0 either
    # way.  A bound inside the table shows it, so the GPU test also runs the production table under a bound of 0.5
    assert not (E.scale_index_ref(s, table, mutant="no_lower_bound") != true).any() and table[0] == np.float32(E.BOUND)
    s2, c2 = E.scale_domain(table, E.INNER_BOUND)
    _populated(c2, E.SCALE_CLASSES, "scale domain, production table, bound 0.5")
    true2 = E.scale_index_ref(s2, table, E.INNER_BOUND)
    assert np.array_equal(true2, R.gc_build_indexes(torch.from_numpy(s2.copy()), torch.from_numpy(table.copy()),
                                                    bound=E.INNER_BOUND).numpy())
    nb = E.scale_index_ref(s2, table, E.INNER_BOUND, mutant="no_lower_bound") != true2
    by = _caught("no_lower_bound", nb, c2, E.SCALE_CLASSES)
    assert by["under-bound"] == int(nb.sum()) > 0 and by["bound"] == 0


def test_the_rounding_mutant_is_caught():
    y, mu, c = E.residual_domain()
    _, sym, y_hat = E.gc_ref(None, mu, None, y=y)
    _, sym_m, y_hat_m = E.gc_ref(None, mu, None, y=y, mutant="round_half_away")
    by = _caught("round_half_away", sym_m != sym, c, E.RES_CLASSES)
    assert by["tie"] > 0 and by["random"] == 0 and by["integer"] == 0
    # ... and the sign of a zero symbol only in y_hat's bits: -0.0 + mu is compared as a pattern
    z, med, cz = E.eb_domain(3, 257)
    by = _caught("round_half_away", E.eb_ref(med, 257, z=z, mutant="round_half_away")[0] != E.eb_ref(med, 257, z=z)[0], cz,
                 E.RES_CLASSES)
    assert by["tie"] > 0 and by["random"] == 0


@pytest.mark.parametrize("which", ["production", "ragged"])
def test_every_resolve_mutant_is_caught(which):
    sym, idx, c, (cdf, lens, offs) = E.resolve_domain(which)
    true = E.resolve_ref(sym, idx, cdf, lens, offs)

    def diff(name):
        m = E.resolve_ref(sym, idx, cdf, lens, offs, mutant=name)
        d = np.zeros(sym.size, dtype=bool)
        for a, b in zip(m[:4], true[:4]):
            d |= a.astype(np.int64) != b.astype(np.int64)
        return d

    by = _caught("compact_gt_4096", diff("compact_gt_4096"), c, E.RESOLVE_CLASSES)
    assert by["payload-edge"] > 0 and by["regular"] == 0
    by = _caught("nibbles_pow16", diff("nibbles_pow16"), c, E.RESOLVE_CLASSES)
    assert by["payload-edge"] > 0 and by["regular"] == 0
    by = _caught("escape_gt_max", diff("escape_gt_max"), c, E.RESOLVE_CLASSES)
    assert by["payload-0"] > 0 and by["payload-0"] == by["escape"]
    by = _caught("payload0_as_0", diff("payload0_as_0"), c, E.RESOLVE_CLASSES)
    assert by["payload-0"] > 0 and by["payload-0"] == by["escape"]
    if which == "ragged":
        # only a bin of frequency 65536 has range bits above the mask, and only arithmetic wider than 32 bits keeps them:
        # packed into a uint32 the shift drops them again (the device's sr is safe either way; the host encoder divides by
        # the range itself, where the mask decides between "refused" and a wrong stream)
        by = _caught("range_unmasked", diff("range_unmasked"), c, E.RESOLVE_CLASSES)
        assert by["full-range-row"] > 0 and by["regular"] == 0 and by["full-range-row"] == by["escape"]
    else:
        assert not diff("range_unmasked").any()


def test_the_reporter_names_position_class_and_inputs():
    y, mu, c = E.residual_domain()
    _, sym, y_hat = E.gc_ref(None, mu, None, y=y)
    n = E.compare_ints(sym.astype(np.int32), sym, c, E.RES_CLASSES, dict(y=y, mu=mu), "sym")
    assert n == sym.size
    _, sym_m, _ = E.gc_ref(None, mu, None, y=y, mutant="round_half_away")
    with pytest.raises(E.IntMismatch) as ei:
        E.compare_ints(sym_m, sym, c, E.RES_CLASSES, dict(y=y, mu=mu), "sym")
    e = ei.value
    print(str(e))
    first = int(np.nonzero(sym_m != sym)[0][0])
    assert e.first == first and "tie" in e.first_classes and e.n == int((sym_m != sym).sum())
    assert f"first at {first}" in str(e) and "y = " in str(e) and "mu = " in str(e)
    # float32 outputs are compared by bit pattern: -0.0 is not +0.0
    a = np.array([0.0, -0.0], dtype=np.float32)
    with pytest.raises(E.IntMismatch):
        E.compare_ints(a, np.zeros(2, dtype=np.float32), np.zeros(2, np.uint8), E.RES_CLASSES, dict(a=a), "zeros")
