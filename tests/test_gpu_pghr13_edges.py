"""GPU tier of the PGHR13 batch-check edge tests (cases: tests/pghr13_edges.py; expectations from the
oracle alone, see there). zg_pghr13_verify accepts every proof of a call on ONE folded check, so what
must hold is (a) the exact statuses and (b) whether that check failed (stats pghr13_batch_failures): a
term dropped from a sum fails the check of an all-valid call although the per-proof rerun still returns
the right statuses, and a slot the check skips accepts a false proof only when no other proof of the call
fails. Both are asserted per call, under every (B, K) launch shape, at ragged sizes, with the one
failing proof in each slot where a lane map ends or wraps, with slots the batch excludes, with nothing
live, over several chunks per call, and on a context that takes its weights from the operating system.

The shape is the context's (ZG_STRAUS_B / ZG_BSEG_K / ZG_PGHR_CHUNK read in zg_create) and
zg_pghr13_shape reports it from the helper the call launches by, so every test first proves that the
shape it means to run is the one that runs."""
import os

import pytest

from tests import pghr13_edges as E

pytestmark = pytest.mark.gpu


def _ctx_env(env, seed=7):
    """a context created under env (the pattern of tests/test_gpu_csum._ctx_env), Groth16 keys not loaded"""
    from zebra_amd import Context
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Context(device=0, max_batch=64, load_builtin=False, seed=seed)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=E.SHAPES, ids=E.shape_id)
def shaped(request):
    c = _ctx_env(request.param)
    yield request.param, c
    c.close()


def _bk(ctx, env, n):
    """the (B, K) of a call of n proofs, as the context reports it -- and as env forces it"""
    got, want = ctx.pghr13_shape(n), E.expected_shape(env, n)
    assert got == want, (n, got, want)
    return got["straus_b"], got["bseg_k"]


def _run(ctx, case, with_time=False):
    """one call -> the oracle's statuses, one more call counted, the batch check failed iff the oracle says
    a proof that takes part is false"""
    st0 = ctx.stats()
    got = ctx.pghr13_verify(case.proofs, case.inputs, case.counts, with_time=with_time)
    st1 = ctx.stats()
    if with_time:
        got, ms = got
        assert ms > 0, case.name
    want = case.statuses
    assert got == want, (case.name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])
    assert st1["pghr13_calls"] - st0["pghr13_calls"] == 1, case.name
    assert st1["pghr13_batch_failures"] - st0["pghr13_batch_failures"] == (1 if case.fails else 0), case.name


def test_forced_shape_is_applied(shaped):
    env, ctx = shaped
    for n in E.SWEEP_SIZES + E.LARGE_SIZES + [0, 65536, 1 << 20]:
        got = ctx.pghr13_shape(n)
        assert got == E.expected_shape(env, n), (n, got)
        if env:
            assert (got["straus_b"], got["bseg_k"]) == (env["ZG_STRAUS_B"], min(32, env["ZG_BSEG_K"]))
        assert got["chunk"] == E.DEFAULT_CHUNK


def test_automatic_shape_thresholds():
    """a default context: K = 1, 2, 4, 8 from 0, 16,384, 32,768, 65,536 proofs, B = 2 from 28,672, two waves
    per proof of the rerun's Miller loop below 32,768, P_i7 on the side stream from there; a larger call's
    shape is its first chunk's. Nothing is launched."""
    ctx = _ctx_env({})
    try:
        for n in E.THRESHOLD_SIZES + [65537, 1 << 24]:
            assert ctx.pghr13_shape(n) == E.expected_shape({}, n), n
        at = lambda n: ctx.pghr13_shape(n)  # noqa: E731
        assert [at(n)["bseg_k"] for n in (0, 16383, 16384, 32767, 32768, 65535, 65536)] == [1, 1, 2, 2, 4, 4, 8]
        assert [at(n)["straus_b"] for n in (28671, 28672)] == [1, 2]
        assert [(at(n)["halves"], at(n)["p7_side"]) for n in (32767, 32768)] == [(2, 0), (1, 1)]
        assert ctx.stats()["pghr13_calls"] == 0
    finally:
        ctx.close()


def test_all_valid_ragged_sweep(shaped):
    """every sweep and large size, all valid, a smaller call after a larger one in the same arena: the batch
    check alone accepts each call; then the large sizes with one mutant in the last slot"""
    env, ctx = shaped
    for n in E.VALID_ORDER:
        _bk(ctx, env, n)
        _run(ctx, E.all_valid(n))
    for n in E.LARGE_SIZES:
        _run(ctx, E.large_bad(n))
        _run(ctx, E.all_valid(n - 2036))      # 27, 2,063: stale pts / status / part beyond the new n


def test_one_bad_proof_per_call(shaped):
    """per sweep size and critical position of this shape's lane maps: that slot alone holds a mutant (the
    class rotating over the five equalities) -> exactly that slot is VERIFY_FAILED and the batch check
    failed; after each size's failing calls an all-valid call of the next smaller size passes on the same
    arena"""
    env, ctx = shaped
    sizes = sorted(E.SWEEP_SIZES, reverse=True)
    for n, smaller in zip(sizes, sizes[1:] + [None]):
        b, k = _bk(ctx, env, n)
        cases = E.position_sweep(n, b, k)
        assert cases and cases[0].names[n - 1] in E.MUTANTS
        for c in cases:
            assert sorted(c.statuses) == [0] * (n - 1) + [3]
            _run(ctx, c)
        if smaller:
            _run(ctx, E.all_valid(smaller))


def test_excluded_slots(shaped):
    """a decode-invalid proof (b outside the subgroup: decided on the side stream) and a row with an input
    >= r in slots 0 and n-1: exact statuses, and the batch check of the others still passes"""
    env, ctx = shaped
    for n in E.SWEEP_SIZES:
        _bk(ctx, env, n)
        for c in E.excluded(n):
            assert not c.fails
            _run(ctx, c)


def test_nothing_live(shaped):
    """no proof reaches the batch check: every operand sum is infinity, no b pair exists, and the product
    over nothing is 1 -- after a failing call, so the arena holds another call's sums"""
    env, ctx = shaped
    _run(ctx, E.one_bad(65, 64, 0))
    for c in E.nothing_live():
        _bk(ctx, env, c.n)
        assert not c.fails and E.OK not in c.statuses
        _run(ctx, c)
    _run(ctx, E.all_valid(5))


@pytest.mark.parametrize("env", E.CHUNK_ENVS, ids=E.shape_id)
def test_chunks(env):
    """ZG_PGHR_CHUNK = 64 (and 1, which clamps to 64): calls of 1, 2, 3 and 4 chunks, the last one ragged;
    one call is counted once and fails once however many chunks it took, the statuses land at their
    chunk's offset and kernel_ms sums the chunks"""
    ctx = _ctx_env(env)
    try:
        for n in E.CHUNK_SIZES:
            assert ctx.pghr13_shape(n) == E.expected_shape(env, n) and ctx.pghr13_shape(n)["chunk"] == 64
            _run(ctx, E.all_valid(n), with_time=True)
            for q, p in enumerate(E.chunk_positions(n)):
                _run(ctx, E.one_bad(n, p, E.mutant_class(n, q)), with_time=True)
    finally:
        ctx.close()


def test_two_chunks_at_the_default_chunk_size():
    """65,536 + 3 proofs on a default context: a full chunk (B = 2, K = 8, P_i7 on the side stream) that
    passes and a chunk of 3 whose last proof fails"""
    ctx = _ctx_env({})
    try:
        n = E.DEFAULT_CHUNK + 3
        assert ctx.pghr13_shape(n) == {"straus_b": 2, "bseg_k": 8, "chunk": 65536, "halves": 1, "p7_side": 1}
        _run(ctx, E.large_bad(n), with_time=True)
    finally:
        ctx.close()


def test_unseeded_context():
    """weights from the operating system (no seed), B = 4 and K = 8: an all-valid call and one with a
    single mutant"""
    env = E.UNSEEDED_SHAPE
    ctx = _ctx_env(env, seed=None)
    try:
        b, k = _bk(ctx, env, 130)
        assert (b, k) == (4, 8)
        _run(ctx, E.all_valid(130))
        _run(ctx, E.position_sweep(130, b, k)[2])
        _run(ctx, E.all_valid(130))
    finally:
        ctx.close()
