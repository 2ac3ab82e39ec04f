"""Shielded transactions from their bytes on the GPU (zg_shielded_verify): statuses, indices,
details, hashes and the per-description classes against tests/shielded_ref.py, exactly. The case list is that of
tests/shielded_cases.py; its reference results are cached per transaction and shared."""
import pytest

from tests import shielded_cases as C
from tests import shielded_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64)


def check(ctx, txs, branch_ids, names=None):
    got = ctx.shielded_verify(txs, branch_ids)
    want = S.run(txs, branch_ids)
    for k, what in enumerate(("tx_status", "status", "index", "detail", "hashes", "desc_status")):
        for t in range(len(txs)):
            assert got[k][t] == want[k][t], (what, t, names[t] if names else None, got[k][t], want[k][t])
    return got


def test_every_case_in_one_call(ctx):
    cs = C.cases()
    got = check(ctx, [c[1] for c in cs], [c[2] for c in cs], [c[0] for c in cs])
    assert set(got[1]) == set(range(8))
    assert set(got[3]) | {d for row in got[5] for d in row} == set(range(20)) - set(S.SHD_UNREACHABLE)


def test_optional_outputs(ctx):
    cs = C.cases()[:8]
    txs, br = [c[1] for c in cs], [c[2] for c in cs]
    full = ctx.shielded_verify(txs, br)
    bare = ctx.shielded_verify(txs, br, want_hashes=False, want_desc=False)
    assert bare[:4] == full[:4] and bare[4] is None and bare[5] is None


@pytest.mark.parametrize("n_desc", [63, 64, 65, 130])
def test_ragged_description_counts(ctx, n_desc):
    """with max_batch = 64 the Groth16 rows cross a batch boundary and a wave boundary; a failing description in the
    first and in the last slot"""
    txs, br = C.window(n_desc)
    got = check(ctx, txs, br)
    assert sum(len(r) for r in got[5]) == n_desc
    assert got[5][0] == [S.SHD_VALUE_COMMITMENT_SMALL_ORDER] and got[5][-1] == [S.SHD_PROOF_INVALID]
    assert set(got[1][1:-1]) == {S.SHTX_OK}


@pytest.mark.parametrize("make", [C.spliced_outputs, C.spliced_joinsplits, C.spliced_spends])
def test_spliced_positions(ctx, make):
    """130 descriptions of one kind in one transaction, the bad one at position 0, 63, 64 and last"""
    pos = (0, 63, 64, 129)
    txs = [make(130, j) for j in pos]
    got = check(ctx, txs, [C.SAPLING_BRANCH] * len(txs))
    for j, row in zip(pos, got[5]):
        assert row[j] != S.SHD_OK and len({c for i, c in enumerate(row[:130]) if i != j}) == 1
    if make is C.spliced_outputs:
        assert got[2] == list(pos) and set(got[1]) == {S.SHTX_INVALID_SAPLING}


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_alignment(ctx, lead):
    """the same window behind a malformed leading slice of 0..3 bytes: every field a lane reads starts at each
    residue mod 4"""
    cs = C.cases()
    txs, br = [bytes(lead)] + [c[1] for c in cs], [0] + [c[2] for c in cs]
    got = check(ctx, txs, br)
    assert got[1][0] == S.SHTX_TX_MALFORMED


def test_nothing_to_launch(ctx):
    cs = {c[0]: c for c in C.cases()}
    pick = [cs[k] for k in ("v1", "v3_none", "v3_host", "truncated", "noncanonical")]
    got = check(ctx, [c[1] for c in pick], [c[2] for c in pick])
    assert got[1] == [S.SHTX_NONE, S.SHTX_NONE, S.SHTX_HOST, S.SHTX_TX_MALFORMED, S.SHTX_TX_NONCANONICAL]
    assert ctx.shielded_verify([], []) == ([], [], [], [], [], [])


def test_needs_the_keys():
    from zebra_amd import Context, zg
    bare = Context(device=0, max_batch=64, load_builtin=False)
    with pytest.raises(zg.ZgError) as e:
        bare.shielded_verify([C.real()["sap0"]], [C.SAPLING_BRANCH])
    assert e.value.code == -3   # ZG_E_NOVK


def test_agrees_with_the_six_call_path(ctx):
    """the verdict of collector.verify_block over host-sliced fields (zg_sighash, zg_prep_batch, zg_verify_batch,
    zg_sapling_bvk, zg_redjubjub_verify, zg_ed25519_verify), transaction by transaction. The collector skips the binding
    check of a v4 transaction without spends and outputs: those are left out"""
    from zebra_amd import collector, zg
    cs = [c for c in C.cases() if S.verify_tx(c[1], c[2])[0] == 0 and S.verify_tx(c[1], c[2])[5]]
    got = ctx.shielded_verify([c[1] for c in cs], [c[2] for c in cs])
    assert len(cs) >= 30
    for k, (name, raw, br) in enumerate(cs):
        err = collector.verify_block([C.collector_tx(raw, br)], ctx=ctx)
        st = got[1][k]
        want = None if st == zg.SHTX_OK else (0, ("InvalidJoinSplit", got[2][k]) if st == zg.SHTX_INVALID_JOINSPLIT
                                              else zg.SHTX_ERRORS[st])
        assert err == want, (name, err, want)
