"""The seams of the one-shot entries' host plumbing on the GPU (zebra_amd/csrc/zg_calls.hip over zg_host.h): calls
with every optional output absent at n = 0, 1 and 65, payloads of no bytes, offset tables that do not start at
zero, the argument rejects of the five offset tables, and the per-context arenas grown, reused and asked for less.
The per-feature suites aim at the kernels; this file aims at what moves their buffers. Expected values are the
references' (tests/*_ref.py, the oracles, the fixtures), and for the arenas also a fresh context's."""
import ctypes
import hashlib
import random

import pytest

from tests import blocks_cases as BC
from tests import blocks_ref as BR
from tests import ecdsa_ref as EC
from tests import sig_edges as E
from tests import sighash_cases as SC
from tests import sighash_ref as SR
from tests.test_equihash import fixture as eq_fixture, h

pytestmark = pytest.mark.gpu

E_INVAL = -1
SIZES = (0, 1, 65)      # nothing, one lane, one wave and one lane
DATA = hashlib.shake_128(b"zg call edges").digest(4096)


def new_ctx(**kw):
    from zebra_amd import Context
    return Context(device=0, max_batch=64, seed=7, load_builtin=False, **kw)


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    c.close()


def L():
    from zebra_amd import zg
    return zg.lib()


def buf(n):
    return ctypes.create_string_buffer(max(n, 1))


def u64s(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def u32s(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


# ---------------------------------------------------------------- optional outputs absent
def header_items(n):
    """n headers cycling the 13 real ones, a mutant in the last place (and the first, from two on) -> the
    serialized headers, (status, flags) and the block hash of each"""
    g = eq_fixture()
    items = [g["real"][i % 13] for i in range(n)]
    want = [(0, 0)] * n
    for k, place in enumerate((-1, 0)[:min(n, 2)]):
        m = g["mutants"][(n + 5 * k) % len(g["mutants"])]
        items[place], want[place] = m, (m["status"], m["flags"])
    return [h(e["header"]) for e in items], want, [h(e["hash"]) for e in items]


@pytest.mark.parametrize("n", SIZES)
def test_equihash_without_repeated(ctx, n):
    from zebra_amd import zg
    from tests import equihash_ref as Q
    hs, want, _ = header_items(n)
    ok = buf(n)
    rc = L().zg_equihash_verify(ctx._p, zg.EQ_200_9, n, b"".join(x[:140] for x in hs) or None, 140,
                                b"".join(x[143:] for x in hs) or None, ok, None)
    assert rc == 0 and list(ok.raw[:n]) == [0 if f & Q.F_EQUIHASH else 1 for _, f in want]
    assert [bool(b) for b in ok.raw[:n]] == ctx.equihash_verify(zg.EQ_200_9, [x[:140] for x in hs], [x[143:] for x in hs])[0]


@pytest.mark.parametrize("n", SIZES)
def test_headers_without_hashes_and_flags(ctx, n):
    hs, want, hashes_want = header_items(n)
    st = buf(n)
    rc = L().zg_headers_verify(ctx._p, n, b"".join(hs) or None, eq_fixture()["max_bits"], st, None, None)
    assert rc == 0 and list(st.raw[:n]) == [s for s, _ in want]
    for hashes, flags in ((buf(32 * n), None), (None, buf(n))):          # and each alone
        assert L().zg_headers_verify(ctx._p, n, b"".join(hs) or None, eq_fixture()["max_bits"], st, hashes, flags) == 0
        assert list(st.raw[:n]) == [s for s, _ in want]
        if flags:
            assert list(flags.raw[:n]) == [f for _, f in want]
        if hashes:
            assert hashes.raw[:32 * n] == b"".join(hashes_want)


@pytest.mark.parametrize("n", SIZES)
def test_jubjub_decode_without_xy(ctx, n):
    pts, want = ([], []) if n == 0 else E.decode_batches()[E.SIZES.index(n)]
    assert len(pts) == n
    st = buf(n)
    assert L().zg_jubjub_decode(ctx._p, n, b"".join(pts) or None, st, None) == 0
    assert list(st.raw[:n]) == [w[0] for w in want]
    assert len(set(st.raw[:n])) >= min(n, 2)       # the statuses differ, so the copy back is seen


def window(n):
    """n serialized blocks: good ones of 1..4 transactions, a block failing a check, a malformed and an empty one"""
    blocks = [BC.synthetic(1 + i % 4, seed=i) for i in range(n)]
    if n > 1:
        blocks[-1] = BC.failing(("merkle",))[0]                    # a wrong root: known only after the hashing
        blocks[n // 2] = blocks[n // 2][:-1]                       # malformed: hashes nothing
        blocks[1] = BR.make_block(BC.header(), [])                 # empty
    return blocks


def want_window(blocks):
    ws = [BR.verify(raw, BC.BIG, BC.BIG) for raw in blocks]
    counts = [0]
    for w in ws:
        counts.append(counts[-1] + len(w[4] or []))
    return ws, counts


@pytest.mark.parametrize("n", SIZES)
def test_blocks_verify_without_flags_detail_roots_txids(ctx, n):
    from zebra_amd import zg
    blocks = window(n)
    ws, counts = want_window(blocks)
    arena, off = zg.pack_slices(blocks)
    st, cnt = buf(n), (ctypes.c_uint64 * (n + 1))(*([99] * (n + 1)))
    rc = L().zg_blocks_verify(ctx._p, n, arena + b"\0", off, BC.BIG, BC.BIG, 0, st, None, None, None, cnt, None)
    assert rc == 0 and list(st.raw[:n]) == [w[0] for w in ws] and list(cnt) == counts
    if n > 1:
        assert len(set(st.raw[:n])) >= 4 and counts[-1] > n
    got = ctx.blocks_verify(blocks, BC.BIG, BC.BIG)                      # and with every output present
    assert got[0] == [w[0] for w in ws] and got[4] == counts
    assert got[3] == [w[3] or bytes(32) for w in ws] and got[5] == [w[4] or [] for w in ws]


# ---------------------------------------------------------------- payloads of no bytes
def ec_keys():
    keys = [EC.pubkey_bytes(EC.mul(d, EC.G), compressed=bool(d & 1)) for d in (3, 4, 0x1234567)]
    return keys + [keys[0][:20]]                                       # and one of a wrong length


def test_ecdsa_with_every_signature_empty(ctx):
    keys = ec_keys()
    pk = [keys[i % len(keys)] for i in range(65)]
    msgs = [DATA[32 * i:32 * i + 32] for i in range(65)]
    want = [EC.verify(k, b"", m) for k, m in zip(pk, msgs)]
    assert sorted(set(want)) == [EC.PUBLIC, EC.SIGNATURE_ENCODING]
    assert ctx.ecdsa_verify(pk, [b""] * 65, msgs) == want


def test_txids_with_an_empty_slice_between_two_others(ctx):
    for slices in ([DATA[:100], b"", DATA[100:177]], [b"", b"", b""], [b"", DATA[:64], b""]):
        assert ctx.txids(slices) == [BR.dhash256(s) for s in slices]


def test_sighash_without_items_and_with_empty_script_codes(ctx):
    txs = SC.small_txs()
    br = SC.branches(txs)
    assert ctx.sighash(txs, br, []) == ([0, 0, 0], [], [])
    items = [(t, i % 2, b"", 1000 + i, ht) for i, (t, ht) in
             enumerate((t, ht) for t in range(3) for ht in SC.HASHTYPE_CLASSES)]
    items = (items * 4)[:65]
    want = SR.run(txs, br, items)
    assert ctx.sighash(txs, br, items) == (want[0], want[1], want[2])
    assert set(want[2]) == {0} and len(set(want[1])) > 10


def test_blocks_verify_window_of_malformed_blocks(ctx):
    good = BC.synthetic(3)
    blocks = [good[:-1], good[:40], b"", BC.noncanonical_count(good, 0xFD), good + b"\0"]
    ws, counts = want_window(blocks)
    assert counts == [0] * 6 and all(w[0] != 0 for w in ws)
    got = ctx.blocks_verify(blocks, BC.BIG, BC.BIG)
    assert got[0] == [w[0] for w in ws] and got[4] == counts and got[1] == [0] * 5
    assert got[3] == [bytes(32)] * 5 and got[5] == [[]] * 5


def test_sapling_bvk_without_any_value_commitment(ctx):
    values = [0, 1, -1, 2 ** 63 - 1, -2 ** 63 + 1, -2 ** 63] + list(range(5, 64))
    want = [E.bvk_expect([], [], v) for v in values]
    assert len(values) == 65 and [w[0] for w in want].count(2) == 1
    assert ctx.sapling_bvk([([], [], v) for v in values]) == want


# ---------------------------------------------------------------- a first offset that is not zero
def test_txids_first_offset_not_zero(ctx):
    cuts = [7, 107, 107, 200, 1333]
    assert ctx.txids(arena=DATA, offsets=cuts) == [BR.dhash256(DATA[a:b]) for a, b in zip(cuts, cuts[1:])]


def test_sighash_both_offset_tables_start_past_zero(ctx):
    from zebra_amd import zg
    txs = SC.small_txs()
    br = SC.branches(txs)
    items = [(t, i, DATA[9 * i:9 * i + 5 + 7 * t], 50 + t, ht) for t in range(3) for i in range(2) for ht in (1, 0x83)]
    want = SR.run(txs, br, items)
    arena, tx_off, branch, item_tx, index, scripts, script_off, amount, hashtype = zg.pack_sighash(txs, br, items)
    n, lead, slead = len(items), 13, 5
    ts, hs, st = buf(3), buf(32 * n), buf(n)
    rc = L().zg_sighash(ctx._p, 3, DATA[:lead] + arena + b"\0", u64s([v + lead for v in tx_off]), branch, n, item_tx,
                        index, DATA[:slead] + scripts + b"\0", u32s([v + slead for v in script_off]), amount, hashtype,
                        ts, hs, st)
    assert rc == 0 and list(ts.raw[:3]) == want[0] and list(st.raw[:n]) == want[2]
    assert [hs.raw[32 * i:32 * i + 32] for i in range(n)] == want[1]


def test_ecdsa_first_offset_not_zero(ctx):
    from zebra_amd import zg
    keys = ec_keys()[:3]
    msgs = [DATA[40 * i:40 * i + 32] for i in range(6)]
    sigs = [EC.der(*EC.sign(d, m)) for d, m in zip((3, 4, 0x1234567) * 2, msgs)]
    sigs[4] = b""
    msgs[5] = msgs[0]                                                   # a signature over another message
    pk = keys * 2
    want = [EC.verify(k, s, m) for k, s, m in zip(pk, sigs, msgs)]
    assert want == [0, 0, 0, 0, EC.SIGNATURE_ENCODING, EC.SIGNATURE]
    kb, lens, sg, off, msg = zg.pack_ecdsa(pk, sigs, msgs)
    st = buf(6)
    assert L().zg_ecdsa_verify(ctx._p, 6, kb, lens, DATA[:11] + sg + b"\0", u32s([v + 11 for v in off]), msg, st) == 0
    assert list(st.raw[:6]) == want


def test_blocks_verify_first_offset_not_zero(ctx):
    from zebra_amd import zg
    blocks = window(5)
    ws, counts = want_window(blocks)
    arena, off = zg.pack_slices(blocks)
    st, fl, roots, cnt = buf(5), buf(5), buf(160), (ctypes.c_uint64 * 6)()
    ids = buf(32 * counts[-1])
    rc = L().zg_blocks_verify(ctx._p, 5, DATA[:21] + arena + b"\0", u64s([v + 21 for v in off]), BC.BIG, BC.BIG,
                              counts[-1], st, fl, None, roots, cnt, ids)
    assert rc == 0 and list(st.raw[:5]) == [w[0] for w in ws] and list(fl.raw[:5]) == [w[1] for w in ws]
    assert list(cnt) == counts and roots.raw[:160] == b"".join(w[3] or bytes(32) for w in ws)
    assert ids.raw[:32 * counts[-1]] == b"".join(b"".join(w[4] or []) for w in ws)


# ---------------------------------------------------------------- argument rejects
DEC = (5, 9, 8, 12)                      # a decreasing pair
OVER = (3, 4, 5, 3 + (1 << 31) + 1)      # a span of 2^31 + 1


def test_offset_tables_are_rejected_before_anything_is_read(ctx):
    """each call returns ZG_E_INVAL from its argument checks: the buffers hold one byte"""
    tiny = buf(1)
    out = buf(256)
    three32, three64 = u32s([0, 0, 0]), u64s([0, 0, 0])
    cnt = (ctypes.c_uint64 * 4)()
    lib = L()
    calls = {
        "sig_off": lambda off: lib.zg_ecdsa_verify(ctx._p, 3, tiny, tiny, tiny, u32s(off), tiny, out),
        "tx_off": lambda off: lib.zg_sighash(ctx._p, 3, tiny, u64s(off), three32, 0, None, None, None, None, None,
                                             None, out, None, None),
        "script_off": lambda off: lib.zg_sighash(ctx._p, 3, tiny, u64s([0, 0, 0, 0]), three32, 3, three32, three32,
                                                 tiny, u32s(off), three64, three32, out, out, out),
        "off": lambda off: lib.zg_txids(ctx._p, 3, tiny, u64s(off), out),
        "blk_off": lambda off: lib.zg_blocks_verify(ctx._p, 3, tiny, u64s(off), BC.BIG, BC.BIG, 0, out, None, None,
                                                    None, cnt, None),
    }
    for name, call in calls.items():
        assert call(DEC) == E_INVAL, name
        assert call((9, 9, 9, 8)) == E_INVAL and call((9, 8, 9, 9)) == E_INVAL, name     # the last pair, the first
    for name in ("tx_off", "off", "blk_off"):
        assert calls[name](OVER) == E_INVAL, name


# ---------------------------------------------------------------- the arenas: grow, reuse, ask for less
ARENA_SIZES = (8, 200, 8)


@pytest.fixture(scope="module")
def fresh():
    """a context per size whose arenas no call has touched"""
    cs = {n: new_ctx() for n in set(ARENA_SIZES)}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def reused():
    c = new_ctx()
    yield c
    c.close()


def test_prep_batch_arena_reuse(reused, fresh):
    from zebra_amd import zg as Z
    from tests.test_gpu_prep_batch import _golden_jobs, _host
    base = _golden_jobs()
    sap = [j for j in base if j[0] <= Z.PREP_KIND_OUTPUT]               # the kernel's rows: the arena is used
    js = [j for j in base if j[0] > Z.PREP_KIND_OUTPUT]                 # the host threads' rows
    assert sap and js
    for k, n in enumerate(ARENA_SIZES):
        jobs = [(js if i % 3 == 2 else sap)[(i + k) % len(js if i % 3 == 2 else sap)] for i in range(n)]
        kinds, fields = bytes(j[0] for j in jobs), b"".join(Z.prep_fields(j[0], *j[1]) for j in jobs)
        rows, codes = reused.prep_batch(kinds, fields)
        assert (rows, codes) == fresh[n].prep_batch(kinds, fields), (k, n)
        for i, (kind, a) in enumerate(jobs):
            code, row = _host(Z, kind, a)
            assert (codes[i], rows[288 * i:288 * i + 288]) == (code, row), (k, n, i)


@pytest.mark.parametrize("kind_name", ["SPROUT", "SAPLING"])
def test_tree_roots_arena_reuse(reused, fresh, kind_name):
    from oracle import merkle as M
    kind = getattr(M, kind_name)
    rnd = random.Random(13)
    for k, n in enumerate(ARENA_SIZES):
        st = M.TreeState(kind, 29)
        leaves = [bytes(rnd.getrandbits(8) for _ in range(31)) + b"\0" for _ in range(n)]
        marks = [n, 0, n // 2, 1]
        want, fin = M.window_roots(st, leaves, marks)
        got = reused.tree_roots(kind, 29, st.serialize(), leaves, marks)
        assert got == (want, fin.serialize()), (k, n)
        assert got == fresh[n].tree_roots(kind, 29, st.serialize(), leaves, marks), (k, n)


def test_pghr13_arena_reuse(reused, fresh):
    from tests import pghr13_edges as P
    for k, n in enumerate(ARENA_SIZES):
        case = P.one_bad(n, n - 1 - k, k) if k else P.all_valid(n)
        want = case.fixture_statuses
        assert want.count(0) == n - (1 if k else 0) and None not in want
        got = reused.pghr13_verify(case.proofs, case.inputs, case.counts)
        assert got == want, (k, n)
        assert got == fresh[n].pghr13_verify(case.proofs, case.inputs, case.counts), (k, n)
