"""The exact encoder problems of tests/exact_encoder.py, proved on the CPU: every case tests/test_gpu_exact_encoders.py runs satisfies the exactness
conditions (a)-(e) (check_exact), its reference does not depend on the summation order, and the generated inputs reach the branches of the binned table
gradient they are meant for (bin_model: the quantities bin_kernel / reduce_kernel branch on, restated).  Run with -s to see the figures per problem."""
import numpy as np
import pytest

import exact_encoder as E

CASES = E.all_cases()


def _id(v):
    return str(v).replace(" ", "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_case_is_exact(case):
    p = E.problem(*case)
    rays = E.rays_for(p.M) if case in E.xyz_cases() else None
    fig = E.check_exact(p, rays)
    print("%s: weights <= %d bits, terms <= %d, gradient rows <= %d, largest row sum 2^%.1f of the 2^18 quanta allowed"
          % (_id(case), fig.w_bits, fig.term_bits, fig.grad_bits, fig.row_sum_log2))
    assert fig.term_bits <= (18 if p.F == 2 else 24)
    for variant in E.variants(case):
        E.check_exact(E.problem(*case, **variant), rays)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_reference_is_order_independent(case):
    """The table gradient re-evaluated in f32, one addend at a time, under two random orders: bit-equal to fp64."""
    p = E.problem(*case)
    want = E.reference(p).gtab
    for seed in (1, 2):
        got = E.f32_reordered_gtab(p, seed)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


def test_chunk_halves_are_problems_of_their_own():
    """The two halves of the chunking test (split mid-tile) add up to the whole in fp64."""
    for kind in ("permuto", "hash"):
        p = E.problem(kind, 6, 2, E.ROWS, E.M_MAIN[kind])
        a, b = E.halves(p)
        assert a.M % E.TS[p.enc] != 0 and a.M + b.M == p.M
        E.check_exact(a)
        E.check_exact(b)
        assert np.array_equal(E.reference(a).gtab + E.reference(b).gtab, E.reference(p).gtab)


GEOMETRY_WANT = {          # (rows, F) -> (shift, NS, NS % 8, rows of the last slice)
    (1 << 12, 2): (12, 1, 1, 4096), (1 << 14, 2): (12, 4, 4, 4096), (1 << 15, 2): (12, 8, 0, 4096), (1 << 16, 2): (12, 16, 0, 4096),
    (3 * 4096 + 1000, 2): (12, 4, 4, 1000), (3001, 2): (12, 1, 1, 3001), (5 * 2048 + 77, 4): (11, 6, 6, 77), (1 << 15, 1): (13, 4, 4, 8192),
    (1 << 10, 2): (12, 1, 1, 1024), (1 << 9, 4): (11, 1, 1, 512), (1 << 15, 4): (11, 16, 0, 2048), (1 << 20, 2): (12, 256, 0, 4096),
}


def test_reduce_geometry_of_the_cases():
    """NS, NS % 8 and the last slice's row count from the restated bin_plan; the restatement agrees with the library's workspace size."""
    from pagnerf_amd import _lib as L
    lib = L.load()
    seen = set()
    for case in CASES:
        kind, Lv, F, rows, M = case
        p = E.problem(*case)
        plan = p.plan
        seen.add((rows, F))
        assert (plan.shift, plan.NS, plan.NS % 8, plan.last_rows) == GEOMETRY_WANT[(rows, F)], case
        up = lambda v: (v + 255) // 256 * 256
        entries = Lv * plan.ntiles * plan.TS * E.NV[p.enc]
        want = up(entries * 4) + up(entries * F * 4) + up(Lv * (plan.NS + 1) * plan.ntiles * 4) + up(Lv * plan.ntiles * 4)
        assert lib.pag_encode_bwd_workspace_bytes(M, Lv, F, E.NV[p.enc], rows) == want, case
    assert seen == set(GEOMETRY_WANT)
    assert {p[0] for p in seen if E.bin_plan(1, p[1], "hash", p[0]).NS == 1} and E.problem(*E.BIG).plan.ntiles == 1025          # > 1024 tiles: a second group of 64 for reduce wave 0
    levels = {c[1] for c in CASES}
    assert {1, 2, 3, 24} <= levels          # head = min(RED_HEAD, L / 3) = 0, 0, 1, 8
    assert [min(E.RED_HEAD, n // 3) for n in (1, 2, 3, 24)] == [0, 0, 1, 8]


def _report(case, l, m):
    seg = m.seg[m.seg > 0]
    print("%s level %d: %d entries; repeats per wave and slot < 8 / >= 8: %d / %d; entries per segment min / median / max %d / %d / %d; streams distinct / shared "
          "%d / %d; chunks three-compare / binary-search %d / %d; one row in one chunk of a shared stream >= %.1f"
          % (_id(case), l, m.entries, int((m.repeats < 8).sum()), int((m.repeats >= 8).sum()), seg.min(), int(np.median(seg)), seg.max(), m.distinct, m.shared,
             m.fast, m.slow, m.hot))


def test_inputs_reach_the_regimes(capsys):
    """Per named problem: which side of every branch of the binned pass its entries take (the figures are printed past the capture)."""
    models = {}
    with capsys.disabled():
        print()
    for case in (("permuto", 6, 2, E.ROWS, E.M_MAIN["permuto"]), ("permuto", 6, 4, E.ROWS, E.M_MAIN["permuto"]), ("hash", 6, 2, E.ROWS, E.M_MAIN["hash"]),
                 ("hash_lo", 6, 2, E.ROWS, E.M_MAIN["hash"]), E.MANY_TILES, E.BIG):
        p = E.problem(*case)
        for l in range(p.L):
            models[case, l] = m = E.bin_model(p, l)
            with capsys.disabled():
                _report(case, l, m)
    for (case, l), m in models.items():
        # run_combine: waves that merge (>= 8 adjacent-equal vertex ids) and waves that take the early return, on every level of every problem
        assert (m.repeats >= 8).any() and (m.repeats < 8).any(), (case, l)
        assert ((m.repeats > 0) & (m.repeats < 8)).any(), (case, l)          # the early return with runs present: they must be emitted unmerged
    main = models[("permuto", 6, 2, E.ROWS, E.M_MAIN["permuto"]), 5]
    assert main.G == 1 and main.distinct and main.shared          # both sides of DISTINCT_SEG on the finest level
    assert main.seg.max() >= 4 * E.DISTINCT_SEG and (main.seg[main.seg > 0] < E.DISTINCT_SEG).any()
    assert models[("permuto", 6, 4, E.ROWS, E.M_MAIN["permuto"]), 0].hot >= 8          # lds_accumulate's wave pre-sum at one tile per reduce wave
    many = [models[E.MANY_TILES, l] for l in range(E.MANY_TILES[1])]
    assert all(m.G == 5 for m in many)
    assert many[0].hot >= 8 and many[0].shared and many[0].distinct          # a hot row in a stream of short segments: the pre-sum, across tiles
    assert all(m.slow > 100 and m.fast > 100 for m in many)                  # chunks with four and more tile boundaries, and with fewer
    big = models[E.BIG, 0]
    assert big.G == 64 and big.slow > 1000 and big.fast > 1000 and big.distinct and big.shared
    # the wave_live skip of the XCD8 layout drops the zero waves' entries (they are zeros in the strided layouts)
    p = E.problem("permuto", 8, 2, E.ROWS, E.M_MAIN["permuto"])
    assert E.bin_model(p, 0, grouped=True).entries < E.bin_model(p, 0).entries
    # one level spreads over every slice; the zero level, tile and waves exist
    assert (main.seg.sum(0) > 0).all() and p.zero_level == 6
    assert not p.g[E.TS["permuto"]:2 * E.TS["permuto"]].any() and not p.g[2 * 64:3 * 64].any() and p.g[:64].any()


def test_positions_hold_the_deliberate_runs():
    """On the coarsest level the constructed rays are runs of equal vertex ids: inside a 16-lane row, across lanes 16, 32 and 48, a whole wave, into the next."""
    p = E.problem("permuto", 6, 2, E.ROWS, E.M_MAIN["permuto"])
    xyz = p.xyz[:E.PERIOD]
    step = np.abs(np.diff(xyz, axis=0)).max(1)
    ray = step <= 2.0 / 64 + 1e-9
    for first, n in ((3, 9), (14, 5), (28, 9), (44, 16), (64, 85), (384, 128)):
        assert ray[first:first + n - 1].all() and step[first:first + n - 1].min() > 0, first
    assert (step[256:262] == 0).all()          # one point, seven times
    idx = E.levels(p)[0].idx[:E.PERIOD]
    same = (idx[1:] == idx[:-1]).any(1)
    assert same[3:11].sum() >= 6 and same[14:18].sum() >= 3 and same[28:36].sum() >= 6 and same[64:148].sum() > 70 and same[127]          # [127]: lane 63 -> lane 0 of the next wave
    assert np.array_equal(p.xyz.astype(np.float16).astype(np.float32), p.xyz)
    pts = {tuple(v) for v in xyz[320:344].tolist()}
    assert (1.0, 1.0, 1.0) in pts and (-1.0, -1.0, -1.0) in pts and (0.0, 0.0, 0.0) in pts
    lv = E.levels(p)[0]
    assert (lv.w[320:344] == 1.0).any()        # a point exactly on a lattice vertex: one weight 1, three 0
    assert ((lv.w[:E.PERIOD] == 0.0).sum(1) == 1).any()          # a point on a face of its simplex
