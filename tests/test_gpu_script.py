"""Pay-to-pubkey-hash and pay-to-pubkey inputs on the GPU (zg_inputs_verify): statuses,
details and hashes against tests/script_ref.py, exactly. The case list is that of tests/script_cases.py (the host
build of the same routines runs it in tests/test_script.py); its reference result is computed once and shared."""
import ctypes
import random

import pytest

from tests import script_cases as C
from tests import script_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64, load_builtin=False)


def check(ctx, txs, br, items, flags, want, names=None):
    got = ctx.inputs_verify(txs, br, items, flags)
    assert got[0] == want[0]
    bad = [(k, names[k] if names else items[k][:2], got[1][k], want[1][k], got[2][k], want[2][k])
           for k in range(len(items)) if (got[1][k], got[2][k], got[3][k]) != (want[1][k], want[2][k], want[3][k])]
    assert not bad, (len(bad), bad[:8])


def subset(case, pick):
    """the items `pick` of a case with the transactions they use, renumbered"""
    txs, br, items, _, want = case
    used = sorted({items[k][0] for k in pick})
    at = {t: j for j, t in enumerate(used)}
    sub = [(at[items[k][0]],) + tuple(items[k][1:]) for k in pick]
    return ([txs[t] for t in used], [br[t] for t in used], sub,
            ([want[0][t] for t in used],) + tuple([w[k] for k in pick] for w in want[1:]))


@pytest.mark.parametrize("flags", [0, R.DERSIG])
def test_every_fixture_in_one_call(ctx, flags):
    txs, br, items, names, want = C.case(flags)
    check(ctx, txs, br, items, flags, want, names)
    assert set(want[1]) == set(range(8)) - ({R.INPUT_SIGNATURE_DER} if not flags else set())


def test_reference_vectors_under_their_own_flags(ctx):
    txs, br, items, flags, want, names = C.reference_vectors()
    for k, (f, w) in enumerate(zip(flags, want)):
        _, st, dt, hs = ctx.inputs_verify(txs, br, [items[k]], f)
        assert st == [w] and dt == [0], names[k]
        assert (hs[0] != R.ZERO) == (w == R.INPUT_OK), names[k]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ragged_splits(ctx, n):
    case = C.case(R.DERSIG)
    order = list(range(len(case[2])))
    random.Random(n).shuffle(order)
    lead = [next(k for k in order if case[4][1][k] == s) for s in range(8)]      # all eight statuses inside one wave
    txs, br, items, want = subset(case, (lead + order * 2)[:n])
    check(ctx, txs, br, items, R.DERSIG, want)
    if n >= 8:
        assert set(want[1]) == set(range(8))


def test_first_and_last_byte_of_the_arena(ctx):
    """a P2PK spend whose script_sig is the last thing but the sequence of the last transaction, a P2PKH spend in the
    first; the arena handed over at an offset (tx_off[0] != 0) and the previous scripts likewise"""
    from zebra_amd import zg
    case = C.case(R.DERSIG)
    names = case[3]
    pick = [names.index("p2pkh/v2/01"), names.index("p2pk/sapling/83"), names.index("pushdata/p2pk/4e")]
    txs, br, items, want = subset(case, pick)
    check(ctx, txs, br, items, R.DERSIG, want)
    arena, tx_off, branch, item_tx, index, prev, prev_off, amount = zg.pack_inputs_verify(txs, br, items)
    ntx, n = len(txs), len(items)
    for pad in (1, 2, 3, 5):
        off = (ctypes.c_uint64 * (ntx + 1))(*[o + pad for o in tx_off])
        poff = (ctypes.c_uint32 * (n + 1))(*[o + pad for o in prev_off])
        ts, st, dt = (ctypes.create_string_buffer(k) for k in (ntx, n, n))
        hs = ctypes.create_string_buffer(32 * n)
        rc = zg.lib().zg_inputs_verify(ctx._p, ntx, b"\xee" * pad + arena, off, branch, n, item_tx, index,
                                       b"\xee" * pad + prev, poff, amount, R.DERSIG, ts, st, dt, hs)
        assert rc == 0 and list(st.raw) == want[1] and list(dt.raw) == want[2]
        assert [hs.raw[32 * i:32 * i + 32] for i in range(n)] == want[3]


def test_script_sig_at_each_alignment(ctx):
    """the same spends behind a slice of 0..3 bytes (no transaction: MALFORMED): every transaction, and with it every
    push a lane reads in place, starts at each residue mod 4"""
    case = C.case(R.DERSIG)
    names = case[3]
    pick = [names.index(k) for k in ("p2pkh/overwinter/01", "p2pk/overwinter/01", "preimage/520", "preimage/55")]
    txs, br, items, want = subset(case, pick)
    for shift in range(4):
        moved = [(t + 1,) + tuple(rest) for t, *rest in items]
        check(ctx, [b"\x00" * shift] + txs, [0] + br, moved, R.DERSIG, ([1] + want[0],) + want[1:])


def test_one_call_mixing_all_eight_statuses(ctx):
    case = C.case(R.DERSIG)
    pick = [next(k for k, s in enumerate(case[4][1]) if s == want) for want in range(8)]
    txs, br, items, want = subset(case, pick)
    assert want[1] == list(range(8))
    check(ctx, txs, br, items, R.DERSIG, want)


def test_host_only_call_launches_nothing(ctx):
    case = C.case(0)
    pick = [k for k, s in enumerate(case[4][1]) if s >= R.INPUT_HOST]
    txs, br, items, want = subset(case, pick)
    assert len(pick) >= 20 and set(want[1]) == {4, 5, 6, 7}
    ctx.inputs_verify(*subset(case, [0])[:3], 0)            # a call that launches: the kernel time is not zero
    assert ctx.last_sig_kernel_ms() > 0
    before = ctx.last_sig_kernel_ms()
    check(ctx, txs, br, items, 0, want)
    assert ctx.last_sig_kernel_ms() == before               # no event was recorded: nothing was launched


def test_empty_calls_and_argument_errors(ctx):
    from zebra_amd import zg
    assert ctx.inputs_verify([], [], []) == ([], [], [], [])
    case = C.case(0)
    txs, br, items, want = subset(case, [0, 1])
    assert ctx.inputs_verify(txs, br, []) == (want[0], [], [], [])
    with pytest.raises(zg.ZgError):
        ctx.inputs_verify(txs, br, [(len(txs), 0, b"", 0)])                 # item_tx >= ntx
    with pytest.raises(zg.ZgError):
        ctx.inputs_verify(txs, br, items, flags=2)                          # an undefined flag bit
    with pytest.raises(zg.ZgError):
        ctx.inputs_verify(txs, br, items, flags=3)
    arena, tx_off, branch, item_tx, index, prev, prev_off, amount = zg.pack_inputs_verify(txs, br, items)
    ntx, n = len(txs), len(items)
    ts, st = ctypes.create_string_buffer(ntx), ctypes.create_string_buffer(n)

    def call(tx_off=tx_off, prev_off=prev_off, arena=arena, prev=prev, st=st, ts=ts):
        return zg.lib().zg_inputs_verify(ctx._p, ntx, arena, tx_off, branch, n, item_tx, index, prev, prev_off, amount, 0,
                                         ts, st, None, None)
    assert call() == 0 and list(st.raw) == want[1]                          # detail and hashes absent
    assert call(prev_off=(ctypes.c_uint32 * 3)(0, 30, 25)) == -1            # ZG_E_INVAL: a decreasing table
    assert call(tx_off=(ctypes.c_uint64 * (ntx + 1))(*([5] + [0] * ntx))) == -1
    assert call(arena=None) == -1 and call(prev=None) == -1 and call(st=None) == -1 and call(ts=None) == -1


def test_detail_and_hashes_are_optional(ctx):
    case = C.case(R.DERSIG)
    txs, br, items, _, want = case
    ts, st, dt, hs = ctx.inputs_verify(txs, br, items, R.DERSIG, want_detail=False, want_hashes=False)
    assert (ts, st, dt, hs) == (want[0], want[1], None, None)
    assert ctx.inputs_verify(txs, br, items, R.DERSIG, want_hashes=False)[2] == want[2]
    assert ctx.inputs_verify(txs, br, items, R.DERSIG, want_detail=False)[3] == want[3]


def test_template_path_agrees_with_the_sighash_and_ecdsa_entries(ctx):
    """the verdicts of the records a host interpreter run would gather, through zg_sighash then zg_ecdsa_verify"""
    from tests import sighash_ref as S
    txs, br, items, _, want = C.case(0)
    rec, at = [], []
    for k, (t, i, pk, amount) in enumerate(items):
        if want[1][k] in (R.INPUT_OK, R.INPUT_EVAL_FALSE) and want[3][k] != R.ZERO:
            sig_script = S.parse(txs[t])[1]["inputs"][i]["script"]
            cls, so, sl, ko, kl = R.classify(sig_script, pk)
            key = sig_script[ko:ko + kl] if cls == R.SCRIPT_P2PKH else pk[ko:ko + kl]
            rec.append((key, sig_script[so:so + sl - 1], (t, i, pk, amount, sig_script[so + sl - 1])))
            at.append(k)
    assert len(rec) > 60
    _, hashes, st = ctx.sighash(txs, br, [r[2] for r in rec])
    assert st == [0] * len(rec) and hashes == [want[3][k] for k in at]
    ec = ctx.ecdsa_verify([r[0] for r in rec], [r[1] for r in rec], hashes)
    assert ec == [want[2][k] for k in at] and [R.INPUT_EVAL_FALSE if e else R.INPUT_OK for e in ec] == [want[1][k] for k in at]


# ------------------------------------------------------------------ the collector
def mixed_window(bump_amount=None):
    """the window of tests/test_gpu_sighash.py with the two Sapling-era P2PKH spends handed over as prevouts (no
    interpreter run, no requests) and the other transactions left on the ecdsa_requests path"""
    from tests.conftest import load_golden
    from tests.test_gpu_sighash import window
    from zebra_amd.collector import Prevout, Tx
    w = window("raw", bump_amount=bump_amount)
    for k, v in enumerate(load_golden("sighash.json")["sapling_spends"]):
        amount = v["amount"] + (1 if bump_amount == k else 0)
        assert w[k].raw == bytes.fromhex(v["tx"]) and len(w[k].ecdsa_requests) == 1
        w[k] = Tx(raw=w[k].raw, branch_id=w[k].branch_id, prevouts=[Prevout(bytes.fromhex(v["script"]), amount)])
    return w


def test_collector_mixed_window_gives_the_verdicts_of_the_request_path():
    from tests.test_gpu_sighash import all_ok, window
    from zebra_amd import Context, zg
    from zebra_amd.collector import verify_block
    c = Context(device=0, max_batch=64, load_builtin=False)
    assert verify_block(window("raw"), verify=all_ok, ctx=c) is None
    w = mixed_window()
    assert [t.prevouts is not None for t in w[:3]] == [True, True, False] and any(t.ecdsa_requests for t in w)
    assert verify_block(w, verify=all_ok, ctx=c) is None
    for k in (0, 1):       # a wrong amount fails that transaction's input 0 on either path (the request path's
        old = verify_block(window("raw", bump_amount=k), verify=all_ok, ctx=c)      # stand-in rerun names index k)
        new = verify_block(mixed_window(bump_amount=k), verify=all_ok, ctx=c)
        assert new == (k, ("Signature", 0, "EvalFalse")) and old[0] == new[0] and old[1][::2] == new[1][::2]
    # an input that is no template is the caller's, loudly
    w = mixed_window()
    w[0].prevouts[0].script_pubkey = b"\xa9\x14" + bytes(20) + b"\x87"
    with pytest.raises(zg.ZgError):
        verify_block(w, verify=all_ok, ctx=c)
