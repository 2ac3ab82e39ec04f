"""P2SH and bare multisig inputs on the GPU (zg_inputs_verify with ZG_SCRIPT_TEMPLATE_MULTISIG):
statuses, details and hashes against tests/multisig_ref.py, exactly. The case list is that of
tests/multisig_cases.py (the host build of the same routines runs it in tests/test_multisig.py); its reference result
is computed once and shared."""
import pytest

from tests import multisig_cases as C
from tests import multisig_ref as M
from tests import script_ref as R
from tests.test_gpu_script import check, subset

pytestmark = pytest.mark.gpu

BIT = M.TEMPLATE_MULTISIG


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64, load_builtin=False)


def rows_of(case, k):
    """the ECDSA rows item k of a case takes"""
    from tests import sighash_ref as S
    txs, _, items, _, want = case
    if want[1][k] > R.INPUT_EVAL_FALSE:
        return 0
    t, i, pk, _ = items[k]
    return M.match(S.parse(txs[t])[1]["inputs"][i]["script"], pk, BIT)[5]


@pytest.mark.parametrize("flags", [BIT, BIT | R.DERSIG])
def test_every_case_in_one_call(ctx, flags):
    txs, br, items, names, want = C.case(flags)
    check(ctx, txs, br, items, flags, want, names)
    assert {R.INPUT_OK, R.INPUT_EVAL_FALSE, R.INPUT_HOST} <= set(want[1])
    assert (R.INPUT_SIGNATURE_DER in want[1]) == bool(flags & R.DERSIG)


def test_reference_vector(ctx):
    from zebra_amd import zg
    txs, br, items, _, _, names = C.reference_vectors()
    k = names.index("test_check_transaction_multisig")
    want = M.verify_input(txs[items[k][0]], br[items[k][0]], *items[k][1:], BIT)
    for flags in (BIT, BIT | R.DERSIG):
        _, st, dt, hs = ctx.inputs_verify(txs, br, [items[k]], flags)
        assert (st, dt, hs) == ([R.INPUT_OK], [0], [want[2]]) and want[2] != R.ZERO
    with pytest.raises(zg.ZgError):
        ctx.inputs_verify(txs, br, [items[k]], 2)
    for flags in (0, R.DERSIG):
        assert ctx.inputs_verify(txs, br, [items[k]], flags)[1:] == ([R.INPUT_HOST], [0], [R.ZERO])


@pytest.mark.parametrize("rows", [63, 64, 65, 130])
def test_ragged_row_counts(ctx, rows):
    """2-of-3 inputs of four rows each behind zero, one or two template rows and, for 63, a 1-of-3 of three: a wave
    edge of the ECDSA kernel falls inside an item's pairs; passing and failing items alternate"""
    case = C.case(BIT | R.DERSIG)
    names = case[3]
    four = [names.index("2of3/%d%d" % (a, c)) for a in range(3) for c in range(3)] + [names.index("mn/p2sh/2-of-3/sapling")]
    assert all(rows_of(case, k) == 4 for k in four)
    lead = {63: ["mn/bare/1-of-3/v2"], 64: [], 65: ["mixed/p2pkh"], 130: ["mixed/p2pk", "mixed/p2pkh"]}[rows]
    pick = [names.index(k) for k in lead]
    pick += [four[j % len(four)] for j in range((rows - sum(rows_of(case, k) for k in pick)) // 4)]
    assert sum(rows_of(case, k) for k in pick) == rows
    txs, br, items, want = subset(case, pick)
    assert {R.INPUT_OK, R.INPUT_EVAL_FALSE} <= set(want[1])
    check(ctx, txs, br, items, BIT | R.DERSIG, want)


def test_redeem_script_at_each_alignment(ctx):
    """the same spends behind a slice of 0..3 bytes (no transaction: MALFORMED): every redeem script, and every push
    a lane reads in place, starts at each residue mod 4"""
    case = C.case(BIT | R.DERSIG)
    names = case[3]
    pick = [names.index(k) for k in ("mn/p2sh/2-of-3/overwinter", "padding/375", "padding/511", "wide/15-of-15/p2sh")]
    txs, br, items, want = subset(case, pick)
    assert want[1] == [R.INPUT_OK] * 4
    for shift in range(4):
        moved = [(t + 1,) + tuple(rest) for t, *rest in items]
        check(ctx, [b"\x00" * shift] + txs, [0] + br, moved, BIT | R.DERSIG, ([1] + want[0],) + want[1:])


def test_the_bit_changes_nothing_for_the_other_templates(ctx):
    from tests import script_cases as SC
    txs, br, items, _, want = SC.case(R.DERSIG)
    pick = [k for k, s in enumerate(want[1]) if s <= R.INPUT_EVAL_FALSE]
    txs, br, items, want = subset(SC.case(R.DERSIG), pick)
    assert len(pick) > 80
    assert ctx.inputs_verify(txs, br, items, BIT | R.DERSIG) == ctx.inputs_verify(txs, br, items, R.DERSIG) == tuple(want)


def test_host_only_call_launches_nothing(ctx):
    case = C.case(BIT)
    pick = [k for k, s in enumerate(case[4][1]) if s >= R.INPUT_HOST]
    txs, br, items, want = subset(case, pick)
    assert len(pick) >= 30 and set(want[1]) == {R.INPUT_HOST, R.INPUT_RANGE}
    ctx.inputs_verify(*subset(case, [0])[:3], BIT)          # a call that launches: the kernel time is not zero
    before = ctx.last_sig_kernel_ms()
    assert before > 0
    check(ctx, txs, br, items, BIT, want)
    assert ctx.last_sig_kernel_ms() == before               # no event was recorded: nothing was launched


def test_collector_window_with_the_bit():
    from zebra_amd import Context, zg
    from zebra_amd.collector import verify_block
    from tests.test_multisig import window
    c = Context(device=0, max_batch=64, load_builtin=False)
    flags = BIT | R.DERSIG
    kw = dict(verify=lambda *a: [], ctx=c)
    w = window(flags)
    assert verify_block(w, script_flags=flags, **kw) is None
    # one signature corrupted: the byte before a multisig input's last signature's hashtype, in the mixed transaction
    from tests import sighash_ref as S
    t = w[1]
    tx = S.parse(t.raw)[1]
    index = next(i for i, p in enumerate(t.prevouts) if M.match(tx["inputs"][i]["script"], p.script_pubkey, BIT)[0] >= 3)
    sig = bytes(tx["inputs"][index]["script"])
    o, l, _ = M.pushes(sig)[1]
    at = t.raw.index(sig) + o + l - 2
    from dataclasses import replace
    bad = replace(t, raw=t.raw[:at] + bytes([t.raw[at] ^ 1]) + t.raw[at + 1:])
    assert verify_block([w[0], bad, w[2]], script_flags=flags, **kw) == (1, ("Signature", index, "EvalFalse"))
    with pytest.raises(zg.ZgError):
        verify_block(w, **kw)
