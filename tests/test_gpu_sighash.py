"""The transaction signature hash on the GPU (zg_sighash): hashes and statuses against
tests/sighash_ref.py, exactly. The case lists are those of tests/sighash_cases.py (the host build of the same
routine runs them in tests/test_sighash.py); their reference results are computed once and shared."""
import random

import pytest

from tests import sighash_cases as C
from tests import sighash_ref as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64, load_builtin=False)


def h(x):
    return bytes.fromhex(x)


def check(ctx, txs, br, items, want):
    got = ctx.sighash(txs, br, items)
    assert got[0] == want[0]
    bad = [(k, items[k][0], items[k][1], len(items[k][2]), hex(items[k][4]), got[2][k], want[2][k])
           for k in range(len(items)) if got[1][k] != want[1][k] or got[2][k] != want[2][k]]
    assert not bad, (len(bad), bad[:8])


def test_every_fixture_vector_in_one_call_and_at_ragged_sizes(ctx):
    txs, br, items, expected = C.fixture_cases()
    check(ctx, txs, br, items, ([0] * len(txs), expected, [0] * len(items)))
    order = list(range(len(items)))
    random.Random(10).shuffle(order)
    sigver = [R.parse(txs[it[0]])[1]["sigver"] for it in items]
    lead = [next(k for k in order if sigver[k] == v) for v in (2, 0, 1)]    # the three versions inside one wave
    for n in (1, 63, 64, 65, 130):
        pick = (lead + order * 2)[:n]
        check(ctx, txs, br, [items[k] for k in pick], ([0] * len(txs), [expected[k] for k in pick], [0] * n))


@pytest.mark.parametrize("name", sorted(C.SYNTHESIZED))
def test_synthesized_cases(ctx, name):
    """block_edge_sweep: every script length 0..300 per signature version and hashtype class; count_edges: 0, 1
    and 253 inputs / outputs; sprout_edges and sapling_edges: the index and list edges; status_plumbing: a
    malformed and a non-canonical transaction among good ones"""
    txs, br, items, want = C.case(name)
    check(ctx, txs, br, items, want)
    if name == "status_plumbing":
        assert want[0] == [0, 1, 0, 2, 0] and sorted(set(want[2])) == [0, 1, 2]
        assert all(hh == R.ZERO for hh, st in zip(want[1], want[2]) if st)
    if name == "sapling_edges":
        assert want[2].count(R.SIGHASH_INPUT_RANGE) == 12


def test_empty_calls_and_argument_errors(ctx):
    import ctypes
    from zebra_amd import zg
    assert ctx.sighash([], [], []) == ([], [], [])
    txs = C.small_txs()
    assert ctx.sighash(txs, C.branches(txs), []) == ([0, 0, 0], [], [])
    with pytest.raises(zg.ZgError):
        ctx.sighash(txs, C.branches(txs), [(3, 0, b"", 0, 1)])          # item_tx >= ntx
    arena, tx_off, branch, item_tx, index, scripts, script_off, amount, hashtype = zg.pack_sighash(
        txs, C.branches(txs), [(0, 0, b"\x51", 0, 1), (1, 0, b"\x52", 0, 1)])
    ts, hs, st = (ctypes.create_string_buffer(k) for k in (3, 64, 2))

    def call(tx_off=tx_off, script_off=script_off, arena=arena, hs=hs):
        return zg.lib().zg_sighash(ctx._p, 3, arena, tx_off, branch, 2, item_tx, index, scripts, script_off, amount,
                                   hashtype, ts, hs, st)
    assert call() == 0
    dec = (ctypes.c_uint64 * 4)(tx_off[0], tx_off[2], tx_off[1], tx_off[3])
    assert call(tx_off=dec) == -1                                        # ZG_E_INVAL: a decreasing table
    assert call(script_off=(ctypes.c_uint32 * 3)(0, 2, 1)) == -1
    assert call(tx_off=(ctypes.c_uint64 * 4)(0, 1, 2, (1 << 31) + 1)) == -1   # more than 2^31 bytes of transactions
    assert call(arena=None) == -1 and call(hs=None) == -1


def test_gpu_sighash_feeds_the_ecdsa_entry(ctx):
    from zebra_amd import zg
    g = load_golden("sighash.json")
    spends = g["sapling_spends"]
    txs = [h(v["tx"]) for v in spends] + [h(v["tx"]) for v in g["legacy"]]
    br = [v["branch_id"] for v in spends] + [0] * len(g["legacy"])
    items = [(k, 0, h(v["script"]), v["amount"], v["hashtype"]) for k, v in enumerate(spends)]
    items += [(k, 0, h(v["script"]), v["amount"] + 1, v["hashtype"]) for k, v in enumerate(spends)]
    items += [(2 + k, 0, h(v["script"]), 0, 1) for k, v in enumerate(g["legacy"])]
    _, hashes, st = ctx.sighash(txs, br, items)
    assert st == [0] * len(items)
    keys, sigs, msgs, want = [], [], [], []
    for k, v in enumerate(spends + spends):
        keys.append(h(v["pubkey"])), sigs.append(h(v["sig"])), msgs.append(hashes[k])
        want.append(zg.ECDSA_OK if k < 2 else zg.ECDSA_SIGNATURE)
    for k, v in enumerate(g["legacy"]):
        for c in v["checks"]:
            keys.append(h(c["pubkey"])), sigs.append(h(c["sig"])), msgs.append(hashes[4 + k])
            want.append(c["status"])
    assert want.count(zg.ECDSA_OK) >= 8
    assert ctx.ecdsa_verify(keys, sigs, msgs) == want


def sapling_sig_items(raw, sighash, bvk):
    t = R.parse(raw)[1]
    items = [(s[96:128], s[320:384], s[96:128] + sighash, 0) for s in t["spends"]]
    return items + [(bvk, t["binding_sig"], bvk + sighash, 1)]


def test_gpu_no_input_sighash_feeds_ed25519_and_redjubjub(ctx):
    g = load_golden("sighash.json")
    bvks = {e["name"]: h(e["bvk"]) for e in load_golden("sapling_sigs.json")["txs"]}
    js, sap = g["joinsplit"], g["sapling"]
    txs = [h(v["tx"]) for v in js + sap]
    _, hashes, st = ctx.sighash(txs, [v["branch_id"] for v in js + sap], [(k, None, b"", 0, 1) for k in range(len(txs))])
    assert st == [0] * len(txs) and len(js) == 3 and len(sap) >= 2
    assert ctx.ed25519_verify([h(v["pubkey"]) for v in js], [h(v["sig"]) for v in js], hashes[:len(js)]) == [0] * len(js)
    items = [it for k, v in enumerate(sap) for it in sapling_sig_items(h(v["tx"]), hashes[len(js) + k], bvks[v["name"]])]
    assert len(items) >= 4
    assert ctx.redjubjub_verify(*[list(x) for x in zip(*items)]) == [True] * len(items)
    flipped = [(vk, sig, msg[:-1] + bytes([msg[-1] ^ 1]), gen) for vk, sig, msg, gen in items]
    assert ctx.redjubjub_verify(*[list(x) for x in zip(*flipped)]) == [False] * len(items)


# ------------------------------------------------------------------ the collector
def window(form, bump_amount=None):
    """the two Sapling-era spends, the legacy transactions, a JoinSplit-bearing and a Sapling transaction, their
    sighashes either left to the collector (`raw`: Tx.raw + ecdsa_requests) or computed here (`host`)"""
    from zebra_amd.collector import EcdsaCheck, EcdsaRequest, JoinSplit, Output, Spend, Tx
    g = load_golden("sighash.json")
    txs = []

    def transparent(raw, branch, checks):
        """checks: (pubkey, sig, script code, hashtype, amount)"""
        if form == "raw":
            tx = Tx(raw=raw, branch_id=branch,
                    ecdsa_requests=[EcdsaRequest(0, pk, sg, code, ht, amt) for pk, sg, code, ht, amt in checks])
        else:
            tx = Tx(ecdsa_checks=[EcdsaCheck(0, pk, sg, R.sighash(raw, 0, code, amt, ht, branch)[0])
                                  for pk, sg, code, ht, amt in checks])
        tx.eval_rerun = lambda lookup, k=len(txs): ("Signature", k, "EvalFalse")
        txs.append(tx)

    for k, v in enumerate(g["sapling_spends"]):
        amt = v["amount"] + (1 if bump_amount == k else 0)
        transparent(h(v["tx"]), v["branch_id"], [(h(v["pubkey"]), h(v["sig"]), h(v["script"]), v["hashtype"], amt)])
    for v in g["legacy"]:
        transparent(h(v["tx"]), 0, [(h(c["pubkey"]), h(c["sig"]), h(v["script"]), 1, 0)
                                    for c in v["checks"] if c["status"] == 0])
    v = g["joinsplit"][0]
    raw = h(v["tx"])
    t = R.parse(raw)[1]
    js = [JoinSplit(bytes(32), bytes(32), [bytes(32)] * 2, [bytes(32)] * 2, [bytes(32)] * 2, 0, 0, bytes(296),
                    groth=False, pghr_ok=True) for _ in t["joinsplits"]]
    spends = [Spend(s[0:32], s[32:64], s[64:96], s[96:128], s[128:320], spend_auth_sig=s[320:384]) for s in t["spends"]]
    outs = [Output(o[0:32], o[32:64], o[64:96], o[756:948]) for o in t["soutputs"]]
    shielded = Tx(js_pubkey=h(v["pubkey"]), js_sig=h(v["sig"]), joinsplits=js, spends=spends, outputs=outs,
                  value_balance=int.from_bytes(t.get("value_balance", bytes(8)), "little", signed=True),
                  binding_sig=t.get("binding_sig"))
    if form == "raw":
        shielded.raw, shielded.branch_id = raw, v["branch_id"]
    else:
        shielded.sighash = h(v["sighash"])
    txs.append(shielded)
    return txs


def all_ok(proofs, kinds, inputs, n_inputs):
    return [0] * len(kinds)


def test_collector_raw_window_gives_the_verdicts_of_the_host_hashed_window():
    from zebra_amd import Context, zg
    from zebra_amd.collector import Tx, verify_block
    c = Context(device=0, max_batch=64, load_builtin=False)
    assert verify_block(window("host"), verify=all_ok, ctx=c) is None
    assert verify_block(window("raw"), verify=all_ok, ctx=c) is None
    for k in (0, 1):       # the amount is part of the Sapling-era hash: a wrong one fails that transaction's check
        want = (k, ("Signature", k, "EvalFalse"))
        assert verify_block(window("host", bump_amount=k), verify=all_ok, ctx=c) == want
        assert verify_block(window("raw", bump_amount=k), verify=all_ok, ctx=c) == want
    # another branch id is another no-input hash: the JoinSplit signature no longer verifies
    w = window("raw")
    w[-1].branch_id ^= 1
    assert verify_block(w, verify=all_ok, ctx=c) == (len(w) - 1, "JoinSplitSignature")
    # a transaction the GPU does not hash is the caller's, loudly
    w = window("raw")
    w[0].raw = w[0].raw[:-1]
    with pytest.raises(zg.ZgError):
        verify_block(w, verify=all_ok, ctx=c)
    # a window that uses neither new field asks for no sighash call
    calls = []
    old = window("host")
    assert verify_block(old, verify=all_ok, ctx=c, sighash=lambda *a: calls.append(a)) is None and calls == []
    assert all(t.raw is None and not t.ecdsa_requests for t in old) and isinstance(old[0], Tx)
