"""The high word of a 64-bit product as v_mul_hi_u32 + two v_mad_u64_u32 (lash_device.h `mul64_word1`): every hash form that takes it —
the deferring HyperMinHash filter (xxh3_128_4b_hmh_rank), the drain's and the plain kernels' full update (xxh3_128_4b_hmh_fast) and both
under hmh_x=low (the `l x MX2` product, xxh3_l_chain_high) — on the smallest genomes that reach each form, image for image against the
oracle and the direct route against the pack-first one.  A wrong bit in that word moves the bucket or the rank of nearly every k-mer, so
equality on 5e4 .. 7e5 distinct hash inputs is a sharp test; the rare-rank paths of the same forms are tests/test_gpu_rare_hashes.py's.
HyperLogLog and UltraLogLog (xxh3_64: both words of the product, not taken through the helper) ride along on 200 kbp so that a later
change of those products finds its cases here.

Each case asserts from the launch counters that the kernel it is meant for ran.  One genome of 700 kbp alone in a batch is cut into
three slices (the planner's smallest slice is 262 144 bases: plan_items, lash_plan.hip), each under the deferring launch's default
threshold of 600 kbp per work item, so the deferring cases set LASH_DEFER_MIN=0 as the other modules' deferring routes do: without it
they would run the plain kernel and prove nothing about the filter."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ALGO = {"hmh": O.HMH, "hll": O.HLL, "ull": O.ULL}
SEED = 42


@pytest.fixture(scope="module")
def ctx():
    import lash_amd
    c = lash_amd.Context(0)
    yield c
    c.set_layout(None)
    c.close()


_CACHE = {}


def _case(an, k, p, n, spec):
    """one genome of n bases and its oracle image under the layout `spec`: made once per module, never written to"""
    import lash_amd
    key = (an, k, p, n, spec)
    if key not in _CACHE:
        arrays = lash_amd.records_to_arrays([[O.synth_genome(4100 + k, n).tobytes()]])
        want = O.sketch_genomes(ALGO[an], k, p, SEED, *arrays, threads=8, layout=O.parse_layout(spec) if spec else None)
        want.setflags(write=False)
        _CACHE[key] = (arrays, want)
    return _CACHE[key]


def _run(ctx, an, k, p, arrays, flags):
    ctx.enable_timing(True)
    got = ctx.sketch_batch(an, k, p, SEED, *arrays, flags=flags)
    tm = ctx.timing()
    ctx.enable_timing(False)
    return got, tm


def _differ(got, want):
    return "%d of %d bytes differ" % (int((got != want).sum()), want.size)


# k = 16: the default bench's kernel; 13 and 21: the k < 16 and k > 16 word bodies around the same hash forms
@pytest.mark.parametrize("spec", [None, "hmh_x=low"])
@pytest.mark.parametrize("k", [16, 13, 21])
def test_hmh_deferring_filter_and_drain(ctx, k, spec, monkeypatch):
    import lash_amd
    arrays, want = _case("hmh", k, 0, 700_000, spec)
    ctx.set_layout(spec)
    try:
        monkeypatch.setenv("LASH_DEFER_MIN", "0")
        got, tm = _run(ctx, "hmh", k, 0, arrays, lash_amd.F_NO_SOLE)
        assert tm["direct_launches"] == 1 and tm["defer_launches"] == 1 and tm["sole_launches"] == 0, tm
        assert tm["kmers"] == 700_000 - k + 1, tm
        assert got.shape == want.shape and np.array_equal(got, want), ("direct, deferring", k, spec, _differ(got, want))
        packed, tm = _run(ctx, "hmh", k, 0, arrays, lash_amd.F_NO_DIRECT | lash_amd.F_NO_SOLE)
        assert tm["direct_launches"] == 0, tm
        assert np.array_equal(packed, want), ("pack first", k, spec, _differ(packed, want))
        assert np.array_equal(got, packed)
    finally:
        ctx.set_layout(None)


@pytest.mark.sole
@pytest.mark.parametrize("spec", [None, "hmh_x=low"])
def test_hmh_plain_fast_form(ctx, spec, monkeypatch):
    """50 kbp: one work item far below the deferring threshold -> every k-mer takes the full update (xxh3_128_4b_hmh_fast[_xlow]) in the
    sliced direct kernel, in the pack-first route and in the persistent small-genome kernel"""
    import lash_amd
    monkeypatch.delenv("LASH_DEFER_MIN", raising=False)
    arrays, want = _case("hmh", 16, 0, 50_000, spec)
    ctx.set_layout(spec)
    try:
        got, tm = _run(ctx, "hmh", 16, 0, arrays, lash_amd.F_NO_SOLE)
        assert tm["direct_launches"] == 1 and tm["defer_launches"] == 0 and tm["sole_launches"] == 0, tm
        assert got.shape == want.shape and np.array_equal(got, want), ("direct, plain", spec, _differ(got, want))
        packed, tm = _run(ctx, "hmh", 16, 0, arrays, lash_amd.F_NO_DIRECT | lash_amd.F_NO_SOLE)
        assert tm["direct_launches"] == 0 and tm["defer_launches"] == 0, tm
        assert np.array_equal(packed, want), ("pack first", spec, _differ(packed, want))
        sole, tm = _run(ctx, "hmh", 16, 0, arrays, 0)
        assert tm["sole_launches"] >= 1 and tm["direct_launches"] == 0, tm
        assert np.array_equal(sole, want), ("persistent kernel", spec, _differ(sole, want))
    finally:
        ctx.set_layout(None)


@pytest.mark.parametrize("an,k,p", [("hll", 21, 14), ("ull", 16, 12)])
def test_hll_ull_64_bit_products(ctx, an, k, p):
    import lash_amd
    arrays, want = _case(an, k, p, 200_000, None)
    got, tm = _run(ctx, an, k, p, arrays, lash_amd.F_NO_SOLE)
    assert tm["direct_launches"] == 1 and tm["sole_launches"] == 0, tm
    assert got.shape == want.shape and np.array_equal(got, want), ("direct", an, _differ(got, want))
    packed, tm = _run(ctx, an, k, p, arrays, lash_amd.F_NO_DIRECT | lash_amd.F_NO_SOLE)
    assert tm["direct_launches"] == 0, tm
    assert np.array_equal(packed, want), ("pack first", an, _differ(packed, want))
