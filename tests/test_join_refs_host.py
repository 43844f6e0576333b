"""The float64 restatements of tests/join_cases.py (dpi_join_bwd, dpi_bn_bwd_apply_fork, dpi_bn_bwd_apply_dual) against independent code:
float64 autograd of the forward expressions y = BN(act(act(BN_a(xa)) + BN_b(T_CH(xb)))) (Block3d) and y = BN(act(act(BN_a(xa)) +
act(BN_b(xb)))) (ResPath3d) built from torch primitives, and elementwise_cases.bn_bwd_apply64 / bn_bwd_partials64 run in sequence; the
size and edge facts every row is named for; and, restatement against restatement, that the device test's checks (join_cases.check_join,
elementwise_cases.check_partials) catch a wrong kernel.  No GPU: dpi_stat_blocks and dpi_join_bwd_ws_doubles are host functions.

Restatement against autograd, measured over the final rows with V >= 1023 (the two differ only by the float32 rounding of the statistics
the kernels are handed, and by the statistics being frozen before a handful of elements is moved off the activations' jumps):
    tensors (dxa, dxb off the fork range, dxf), norm-wise      max 5.93e-6  (C5-V1287-f3_5-block-t: one element of 6435 moved)
    per-channel vectors (rows of dgb, dgb_f), norm-wise        max 6.42e-6  (the same row, dbeta_b)
Rows without a moved element agree to 6e-7 / 1.1e-6.  Bars: four times the measured maxima (the rounding of the statistics varies with the
seed), AUTOGRAD_T = 2.4e-5 and AUTOGRAD_V = 2.6e-5 below; the measured maxima stay under 2e-5, a tenth of the device test's bar for the
per-channel vectors — otherwise the restatement would be wrong."""
import pytest
import torch

import elementwise_cases as E
import join_cases as J

F64 = torch.float64
MEASURED_T, MEASURED_V = 5.93e-6, 6.42e-6
AUTOGRAD_T, AUTOGRAD_V = 4 * MEASURED_T, 4 * MEASURED_V
GENUINE = [r for r in J.JOIN_ROWS if r.V >= 1023 and r.io == 0]


@pytest.fixture(scope="module")
def L():
    from deep_prior_interpolation_amd import _lib
    return _lib.load()


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _as_launch(ref):
    """The restatement's outputs as a launch would leave them: fp32 tensors and vectors."""
    f = lambda t: None if t is None else t.float()
    return {k: f(ref[k]) for k in ("dxa", "dxb", "dxf", "dgb", "dgb_f")}


# ---- the restatement against float64 autograd -------------------------------------------------------------------------------------------
_worst = {"t": 0.0, "v": 0.0}


@pytest.mark.parametrize("row", GENUINE, ids=J.join_id)
def test_join_restatement_against_float64_autograd(row):
    p = J.join_problem(row)
    ref, auto = J.join_ref(p), J.join_autograd64(p)
    lo, hi = row.fork
    keep = [c for c in range(row.C) if not lo <= c < hi]
    ts = [E.rel(ref["dxa"], auto["dxa"])]
    if keep:
        ts.append(E.rel(ref["dxb"][keep], auto["dxb"][keep]))
    vs = [E.rel(ref["dgb"][i], auto["dgb"][i]) for i in range(6)]
    if row.null_gb:                       # gamma_b = beta_b = NULL: no such parameters, and rows 4, 5 are what they would receive at (1, 0)
        assert p["B"]["gamma"] is None and p["B"]["beta"] is None
    if hi > lo:
        assert bool(torch.isnan(ref["dxb"][lo:hi]).all()) and bool(torch.isnan(auto["dxb"][lo:hi]).all())
        ts.append(E.rel(ref["dxf"], auto["dxf"]))
        vs += [E.rel(ref["dgb_f"][i], auto["dgb_f"][i]) for i in range(2)]
    _worst["t"], _worst["v"] = max(_worst["t"], max(ts)), max(_worst["v"], max(vs))
    print("%s: tensors %.3g, vectors %.3g" % (J.join_id(row), max(ts), max(vs)))
    assert max(ts) <= AUTOGRAD_T and max(vs) <= AUTOGRAD_V, (max(ts), max(vs))
    # the magnitudes bound the values they belong to
    assert bool((ref["mag_dgb"] >= ref["dgb"].abs() * (1 - 1e-12)).all())


def test_the_autograd_bars_are_four_times_the_measured_maxima_and_a_tenth_of_the_device_bar():
    print("worst over the rows run so far: tensors %.3g, vectors %.3g" % (_worst["t"], _worst["v"]))
    assert AUTOGRAD_T == 4 * MEASURED_T and AUTOGRAD_V == 4 * MEASURED_V
    assert 0 < MEASURED_T < 2e-5 and 0 < MEASURED_V < 2e-5 == J.VEC_BAR / 10


def test_stored_t_and_recomputed_t_are_the_same_restatement():
    """t handed as the fp32 of the forward sum, or re-formed in float64 from the two sides: the same gradients to fp32 rounding of t."""
    rows = {(r.C, r.fork): r for r in J.JOIN_ROWS if r.V == 16385 and r.io == 0 and not r.t_stored}
    for row in rows.values():
        stored = J.join_problem(row._replace(t_stored=True))
        p = dict(J.join_problem(row._replace(t_stored=True)), t=None)
        a, b = J.join_ref(stored), J.join_ref(p)
        assert E.rel(a["dxa"], b["dxa"]) < 1e-6 and E.rel(a["dgb"], b["dgb"]) < 1e-5


# ---- fork64 / dual64 against the two-phase restatements run in sequence ------------------------------------------------------------------
@pytest.mark.parametrize("form", range(3))
@pytest.mark.parametrize("V", [5, 1287, 16385])
def test_fork64_against_the_two_phase_restatements(V, form):
    p = J.fork_problem(V, 0, form)
    S, A, B = p["S"], p["A"], p["B"]
    part, _ = E.bn_bwd_partials64(p["dy"], p["x"], S["mi"], S["gamma"], S["beta"], S["chain"], S["pre"], S["post"])
    dx, dg, db = J.fork64(p["dy"], p["x"], S["mi"], S["gamma"], S["beta"], S["chain"], S["pre"], S["post"], part.sum(0))
    dx2, dg2, db2 = E.bn_bwd_apply64(p["dy"], p["x"], S["mi"], S["gamma"], S["beta"], S["chain"], S["pre"], S["post"], part.sum(0))
    assert E.rel(dx, dx2) < 1e-12 * (100 if V <= 5 else 1) and torch.equal(dg, dg2) and torch.equal(db, db2)
    if V > 5:                            # genuine statistics: the header's formula is the gradient itself
        want = E.bn_bwd_autograd64(p["dy"], p["x"], S["gamma"], S["beta"], S["chain"], S["pre"], S["post"])
        assert E.rel(dx, want[0]) < 2e-6 and E.rel(dg, want[1]) < 2e-6 and E.rel(db, want[2]) < 2e-6
    given = dx.float()                   # a follow-up takes its rows of the dx it is GIVEN
    for side in (A, B):
        xs = p["xa"] if side is A else p["xb"]
        ref, mag = J.followup64(given, xs, side["mi"], side["gamma"], side["beta"], side["chain"], side["post"])
        ref2, mag2 = E.bn_bwd_partials64(given, xs, side["mi"], side["gamma"], side["beta"], side["chain"], 1.0, side["post"])
        assert ref.shape == (E.stat_blocks(3, V), 3, 2) and E.rel(ref, ref2) < 1e-12 and E.rel(mag, mag2) < 1e-12
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("C,fork", J.LAYOUTS)
def test_dual64_against_the_two_phase_restatements(C, fork):
    for form in ("block", "respath"):
        p = J.dual_problem(C, 1287, fork, form, 0)
        A, B, fk = p["A"], p["B"], p["fork"]
        assert (fk["lo"], fk["hi"]) == fork and (fk["mi"] is not None) == (fork[1] > fork[0])
        tot = [E.bn_bwd_partials64(p["dy"], x, s["mi"], s["gamma"], s["beta"], s["chain"], 1.0, s["post"])[0].sum(0)
               for x, s in ((p["xa"], A), (p["xb"], B))]
        (dxa, dga, dba), (dxb, dgb, dbb) = J.dual64(p["dy"], A, p["xa"], tot[0], B, p["xb"], tot[1])
        for (dx, dg, db), x, s, t_ in ((((dxa, dga, dba)), p["xa"], A, tot[0]), ((dxb, dgb, dbb), p["xb"], B, tot[1])):
            want = E.bn_bwd_apply64(p["dy"], x, s["mi"], s["gamma"], s["beta"], s["chain"], 1.0, s["post"], t_)
            assert E.rel(dx, want[0]) < 1e-9 and torch.equal(dg, want[1]) and torch.equal(db, want[2])
        if fork[1] > fork[0]:
            lo, hi = fork
            ref, mag = J.dual_fork_partials64(dxb.float(), p["xb"], fk)
            ref2, _ = E.bn_bwd_partials64(dxb.float()[lo:hi], p["xb"][lo:hi], fk["mi"], fk["gamma"], fk["beta"], None, 1.0, fk["post"])
            assert ref.shape == (1, hi - lo, 2) and E.rel(ref, ref2) < 1e-12


# ---- what every row is named for -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", J.JOIN_ROWS, ids=J.join_id)
def test_join_rows_sit_off_the_jumps_and_size_their_workspace(L, row):
    p = J.join_problem(row)
    ma, mb = J.join_edges(p)
    assert int(ma.sum()) == 0 and int(mb.sum()) == 0 and p["nudged"][-1] == 0, p["nudged"]
    nblk = L.dpi_stat_blocks(row.C, row.V)
    assert nblk == E.stat_blocks(row.C, row.V)
    assert L.dpi_join_bwd_ws_doubles(row.C, row.V) == nblk * row.C * J.JOIN_SUMS
    lo, hi = row.fork
    assert 0 <= lo <= hi <= row.C and (p["fork"]["mi"] is None) == (lo == hi)
    if row.io & 1:
        for k in ("xa", "xb", "t"):
            assert p[k] is None or torch.equal(p[k], p[k].to(torch.bfloat16).float()), k
    if row.io & 2:
        assert torch.equal(p["dy"], p["dy"].to(torch.bfloat16).float())
    if row.form == "block":               # chain_b is the identity off the fork range, BN_f + act on it; fwd_chain_b its composition with BN_b
        ident = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0])
        ch = p["B"]["chain"]
        assert all(torch.equal(ch[c], ident) != (lo <= c < hi) for c in range(row.C))
        u = E.chain64(p["xb"], ch)
        g = torch.ones(row.C) if p["B"]["gamma"] is None else p["B"]["gamma"]
        b = torch.zeros(row.C) if p["B"]["beta"] is None else p["B"]["beta"]
        a = (g * p["B"]["mi"][1]).double()[:, None]
        bn = a * u + (b.double() - p["B"]["mi"][0].double() * a[:, 0])[:, None]
        assert E.rel(E.chain64(p["xb"], p["fwd_b"]), bn) < 1e-6
    else:
        assert p["B"]["chain"] is None and p["B"]["post"] == J.SLOPE and p["A"]["post"] == J.SLOPE and lo == hi
    assert (p["t"] is not None) == row.t_stored


def test_named_rows_reach_the_edges_they_are_named_for(L):
    assert J.JOIN_V == tuple(r.V for r in E.V_ROWS)
    assert set(J.KEY_V) == {r.V for r in E.V_ROWS_BF16}
    g = J.group_trips
    for V in (1, 3, 4, 5, 1023):
        assert g(V)[(0, 1)] == 0 and len(g(V)) == 2                                          # first group only
    assert g(1023)[(0, 0)] == 256 and 1023 - 255 * 4 == 3
    t = g(1287)                                                                              # second group for threads 0..65, a 3-element tail
    assert t[(0, 0)] == 256 and t[(0, 1)] == 66 and 1287 - 1024 - 65 * 4 == 3 and len(t) == 2
    assert all(n == 256 for n in g(16384).values()) and len(g(16384)) == 16
    for V in (16385, 16388):
        t = g(V)
        assert E.stat_blocks(1, V) == 2 and t[(4, 0)] == 1 and t[(4, 1)] == 0 and t[(3, 1)] == 256
    t = g(32772)
    assert E.stat_blocks(1, 32772) == 3 and t[(5, 0)] == 171 and t[(5, 1)] == 0 and t[(4, 1)] == 256
    assert E.stat_blocks(1, 49153) == 4 and 49153 % 4 == 1 and g(49153)[(5, 1)] == 256 and g(49153)[(6, 0)] == 1
    # the second-group mutation removes something at exactly the sizes whose second group runs
    for V in J.JOIN_V:
        assert bool((J.group2_keep(V) == 0).any()) == (V > 1024), V
    # layouts
    assert J.LAYOUTS == ((5, (3, 5)), (5, (1, 2)), (3, (0, 3)), (4, (0, 0)), (4, (2, 2)))
    for V in J.JOIN_V:
        have = {(r.C, r.fork) for r in J.JOIN_ROWS if r.V == V and r.io == 0}
        assert len(have) >= 2 and (V not in J.KEY_V or have == set(J.LAYOUTS))
    assert {(r.C, r.fork) for r in J.JOIN_ROWS if r.V <= 5} == set(J.LAYOUTS)
    for V in J.KEY_V:
        rows = [r for r in J.JOIN_ROWS if r.V == V]
        assert {r.io for r in rows} == {0, 1, 2, 3}
        assert {(r.fork, r.t_stored) for r in rows if r.io == 0} == {(f, s) for _, f in J.LAYOUTS for s in (True, False)}
        assert {r.io for r in J.FORK_ROWS if r.V == V} == {0, 1, 2, 3} == {r.io for r in J.DUAL_ROWS if r.V == V}
        assert {(r.form, r.follow) for r in J.FORK_ROWS if r.V == V and r.io == 0 and r.nblk is None} >= {(f, o) for f in range(3) for o in J.FORK_FOLLOW}
        assert {(r.C, r.fork) for r in J.DUAL_ROWS if r.V == V and r.io == 0} == set(J.LAYOUTS)
    assert {r.pre for r in J.JOIN_ROWS} == {J.SLOPE, 1.0} and {r.form for r in J.JOIN_ROWS} == {"block", "respath"}
    assert sum(r.null_gb for r in J.JOIN_ROWS) == 1 and sum(r.null_dgb for r in J.FORK_ROWS) == 1
    assert {r.V for r in J.FORK_ROWS} == set(J.JOIN_V) == {r.V for r in J.DUAL_ROWS}
    assert {r.form for r in J.DUAL_ROWS} == {"block", "respath"}
    for rows in (J.FORK_ROWS, J.DUAL_ROWS):
        assert tuple(r.nblk for r in rows if r.nblk is not None) == E.APPLY_NBLK == (1, 63, 64, 65, 2048)
        assert all(r.V == 1287 for r in rows if r.nblk is not None)
    # the large row
    r = J.LARGE_ROW
    assert r.C == 1 and r.V == E.LARGE_V and not r.t_stored and r.fork == (0, 1) and r.io == 0
    assert r.C * r.V >= E.NT_MIN_FLOATS and L.dpi_stat_blocks(1, r.V) == E.MAX_STAT_BLOCKS
    assert -(-E.stat_span(r.V, E.MAX_STAT_BLOCKS) // 1024) == 17 and -(-(-(-r.V // 32)) // 256) > E.EW_MAX_BLOCKS
    assert L.dpi_join_bwd_ws_doubles(1, r.V) == E.MAX_STAT_BLOCKS * J.JOIN_SUMS


@pytest.mark.parametrize("row", [r for r in J.FORK_ROWS if r.nblk is None and not r.null_dgb], ids=J.fork_id)
def test_fork_rows_sit_off_the_jumps(row):
    p = J.fork_problem(row.V, row.io, row.form)
    assert [int(m.sum()) for m in J.fork_edges(p)] == [0, 0, 0] and p["nudged"][-1] == 0
    assert torch.equal(p["B"]["chain"][0], torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0])) and float(p["B"]["chain"][1, 2]) != 1.0


@pytest.mark.parametrize("row", [r for r in J.DUAL_ROWS if r.nblk is None], ids=J.dual_id)
def test_dual_rows_sit_off_the_jumps(row):
    p = J.dual_problem(row.C, row.V, row.fork, row.form, row.io)
    assert int(J.join_edges(p)[1].sum()) == 0 and p["nudged"][-1] == 0
    A, B = p["A"], p["B"]
    assert int(J.out_edge(p["xa"], A["mi"], A["gamma"], A["beta"], None).sum()) == 0
    assert (A["post"], B["post"]) == ((J.SLOPE, 1.0) if row.form == "block" else (J.SLOPE, J.SLOPE))


# ---- a wrong kernel is caught: the device test's checks on mutated restatements ------------------------------------------------------------
MUTATION_ROWS = [r for r in J.JOIN_ROWS if r.io == 0 and not r.null_gb and r.V in (1, 5, 1023, 1287, 16385, 49153)]


@pytest.mark.parametrize("row", MUTATION_ROWS, ids=J.join_id)
def test_mutated_restatements_fail_the_checks_of_the_device_test(row):
    p = J.join_problem(row)
    ref = J.join_ref(p)
    lo, hi = row.fork
    check = lambda got: J.check_join(_as_launch(got), ref, lo, hi, row.V)
    check(ref)                                                                               # the checks pass on the restatement rounded to fp32
    assert set(J.MUTATIONS) == {"group2_dropped", "fork_index_c", "fork_to_dxb"}
    # a dropped second group: caught wherever the second group has elements, and only there
    assert _fails(lambda: check(J.join_ref(p, "group2_dropped"))) == (row.V > 1024)
    # the fork's constants read at c: caught on every fork range that does not start at channel 0
    assert _fails(lambda: check(J.join_ref(p, "fork_index_c"))) == (hi > lo and lo > 0)
    # the fork's result written into dxb: caught on every fork range
    assert _fails(lambda: check(J.join_ref(p, "fork_to_dxb"))) == (hi > lo)
    if hi > lo:
        bad = _as_launch(J.join_ref(p, "fork_to_dxb"))
        assert not bool(torch.isnan(bad["dxb"][lo:hi]).any()) and bool(torch.isnan(bad["dxf"]).all())


def test_the_mutation_rows_cover_every_layout_on_both_sides_of_the_second_group():
    for big in (False, True):
        assert {(r.C, r.fork) for r in MUTATION_ROWS if (r.V > 1024) == big} == set(J.LAYOUTS)


def test_a_follow_up_row_of_the_wrong_span_fails_the_partial_check():
    """The follow-up partial rows of fork / dual are held with elementwise_cases.check_partials (k = 4, 10) against float64 span sums of
    the stored dx: a span boundary moved by four elements fails it, the fp32-rounded terms pass."""
    p = J.fork_problem(16385, 0, 0)
    A = p["A"]
    dx = torch.randn(p["x"].shape, generator=torch.Generator().manual_seed(1))
    ref, mag = J.followup64(dx, p["xa"], A["mi"], A["gamma"], A["beta"], None, A["post"])
    k = torch.tensor([4.0, 10.0], dtype=F64)
    E.check_partials(ref.clone(), ref, mag, k, "unmutated")
    moved, _ = E.bn_bwd_partials64(dx, p["xa"], A["mi"], A["gamma"], A["beta"], None, 1.0, A["post"], mutation="span_start+4")
    assert _fails(lambda: E.check_partials(moved, ref, mag, k, "span start + 4"))
