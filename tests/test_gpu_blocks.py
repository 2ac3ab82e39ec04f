"""Block bodies on the GPU (zg_txids, zg_blocks_verify): ids, roots, statuses and flags
against tests/blocks_ref.py (hashlib), exactly. The synthetic blocks are those of tests/blocks_cases.py."""
import hashlib
import os

import pytest

from tests import blocks_cases as C
from tests import blocks_ref as R

pytestmark = pytest.mark.gpu

DATA = hashlib.shake_128(b"zg gpu blocks").digest(80000)
EDGE_LENGTHS = (0, 1, 15, 16, 17, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129)


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64, load_builtin=False)


def want_ids(slices):
    return [R.dhash256(s) for s in slices]


def check_txids(ctx, slices):
    got = ctx.txids(slices)
    bad = [(k, len(slices[k])) for k in range(len(slices)) if got[k] != R.dhash256(slices[k])]
    assert not bad, (len(bad), bad[:8])


def test_txids_every_length_0_to_200(ctx):
    check_txids(ctx, [DATA[3 * n:3 * n + n] for n in range(201)])


def test_txids_padding_edges_at_every_start_alignment(ctx):
    """one arena cut into pieces: a filler up to the next wanted residue mod 16, then the slice"""
    arena, cuts, wanted = bytearray(), [0], set()
    for n in EDGE_LENGTHS:
        for a in range(16):
            arena += b"\x5a" * ((a - len(arena)) % 16)
            cuts.append(len(arena))
            arena += DATA[a + 7 * n:a + 7 * n + n]
            cuts.append(len(arena))
            wanted.add((a, n))
    got = ctx.txids(arena=bytes(arena), offsets=cuts)
    assert wanted <= {(a % 16, b - a) for a, b in zip(cuts, cuts[1:])}
    bad = [(a % 16, b - a) for a, b, g in zip(cuts, cuts[1:], got) if g != R.dhash256(bytes(arena[a:b]))]
    assert not bad, bad[:8]


def test_txids_first_and_last_byte_of_the_arena_and_wave_sizes(ctx):
    for n in (1, 63, 64, 65, 130):
        slices = [DATA[100 * i:100 * i + 37 + (i * 29) % 150] for i in range(n)]
        check_txids(ctx, slices)     # slice 0 starts on the arena's first byte, the last ends on its last
    check_txids(ctx, [DATA[:64]])
    check_txids(ctx, [b"", DATA[:1]])
    assert ctx.txids([]) == []


def test_txids_long_slices_among_short_ones_and_the_host_threshold(ctx):
    slices = [DATA[i:i + 90 + i] for i in range(40)] + [DATA[5:5 + 4097]] + [DATA[200 + i:300 + 2 * i] for i in range(30)] \
        + [DATA[9:9 + 70001]] + [DATA[i:i + 127] for i in range(20)]
    want = want_ids(slices)
    assert ctx.txids(slices) == want
    # the same calls on contexts created with ZG_TXID_HOST_MIN=0 (every slice on the device) and =128 (most of them
    # on host threads): the knob is read at zg_create
    from zebra_amd import Context
    blocks = [C.synthetic(3), R.make_block(C.header(), [R.min_tx(0, coinbase=True), R.min_tx(1, out_script=DATA[:3000])])]
    for knob in ("0", "128"):
        os.environ["ZG_TXID_HOST_MIN"] = knob
        try:
            ctx2 = Context(device=0, max_batch=64, load_builtin=False)
        finally:
            del os.environ["ZG_TXID_HOST_MIN"]
        assert ctx2.txids(slices) == want, knob
        assert ctx2.blocks_verify(blocks, C.BIG, C.BIG) == ctx.blocks_verify(blocks, C.BIG, C.BIG), knob
        assert verify(ctx2, blocks)[0] == [0, 0]
        ctx2.close()


def verify(ctx, blocks, limits=None):
    """one call against the restatement, block by block -> what the call returned"""
    max_size, max_sigops = limits or (C.BIG, C.BIG)
    st, fl, det, roots, counts, ids = ctx.blocks_verify(blocks, max_size, max_sigops)
    rows = 0
    for b, raw in enumerate(blocks):
        w = R.verify(raw, max_size, max_sigops)
        assert (st[b], fl[b], det[b]) == w[:3], (b, st[b], fl[b], det[b], w[:3])
        assert roots[b] == (w[3] or bytes(32)) and ids[b] == w[4], b
        assert counts[b] == rows
        rows += len(w[4])
    assert counts[-1] == rows
    return st, fl, det, roots, counts, ids


def test_every_fixture_block_alone_and_all_in_one_call(ctx):
    blocks = [raw for _, raw, _ in C.fixtures()]
    for raw in blocks:
        assert verify(ctx, [raw])[0] == [0]
    st, _, _, roots, counts, _ = verify(ctx, blocks)
    assert st == [0] * len(blocks) and roots == [raw[36:68] for raw in blocks]
    assert counts[-1] == sum(e["layout"][0] for _, _, e in C.fixtures())


@pytest.mark.parametrize("ks", [tuple(range(1, 18)), (255, 256, 257), (1025,)])
def test_synthetic_blocks_of_k_transactions(ctx, ks):
    """1,025: more nodes in the first level than the workgroup has lanes"""
    st = verify(ctx, [C.synthetic(k, seed=k) for k in ks])[0]
    assert st == [0] * len(ks)


def test_65_blocks_with_wrong_roots_at_the_first_the_64th_and_the_last(ctx):
    blocks = [C.synthetic(1 + k % 5, seed=k) for k in range(65)]
    for k in (0, 63, 64):
        b = bytearray(blocks[k])
        b[40] ^= 1
        blocks[k] = bytes(b)
    st, fl = verify(ctx, blocks)[:2]
    assert [k for k in range(65) if st[k]] == [0, 63, 64] and {st[k] for k in (0, 63, 64)} == {R.BLK_MERKLE_ROOT}
    assert [fl[k] for k in (0, 63, 64)] == [R.F_MERKLE_ROOT] * 3


@pytest.mark.parametrize("name,case", C.failing_cases(), ids=["+".join(n) or "good" for n, _ in C.failing_cases()])
def test_each_check_failing_alone_in_pairs_and_all_at_once(ctx, name, case):
    raw, max_size, max_sigops, flags = case
    st, fl, det = verify(ctx, [C.synthetic(2), raw, C.synthetic(3, seed=1)], (max_size, max_sigops))[:3]
    assert fl[1] == flags and (st[1] == 0) == (flags == 0)


def test_malformed_noncanonical_and_empty_blocks_among_good_ones(ctx):
    good = [C.synthetic(3, seed=s) for s in range(4)]
    blocks = [good[0], good[1][:-1], good[1], C.noncanonical_count(good[2], 0xFD), C.failing(("empty",))[0], good[3],
              b"", good[2] + b"\x00"]
    st, _, _, _, counts, ids = verify(ctx, blocks)
    assert st == [0, R.BLK_MALFORMED, 0, R.BLK_NONCANONICAL, R.BLK_EMPTY, 0, R.BLK_MALFORMED, R.BLK_MALFORMED]
    assert counts == [0, 3, 3, 6, 6, 6, 9, 9, 9] and [len(i) for i in ids] == [3, 0, 3, 0, 0, 3, 0, 0]


def test_nomem_with_the_counts_filled_in_and_empty_calls(ctx):
    from zebra_amd import zg
    blocks = [C.synthetic(3), C.synthetic(4, seed=1)]
    with pytest.raises(zg.ZgError) as e:
        ctx.blocks_verify(blocks, C.BIG, C.BIG, txid_cap=6)
    assert e.value.code == zg.E_NOMEM and e.value.counts == [0, 3, 7]
    assert ctx.blocks_verify(blocks, C.BIG, C.BIG, txid_cap=7)[0] == [0, 0]
    assert ctx.blocks_verify(blocks, C.BIG, C.BIG, txid_cap=0, want_ids=False)[:1] == ([0, 0],)
    assert ctx.blocks_verify([], C.BIG, C.BIG) == ([], [], [], [], [0], [])
    import ctypes
    arena, off = zg.pack_slices(blocks)
    off[1], off[2] = off[2], off[1]      # a decreasing offset table
    st, cnt = ctypes.create_string_buffer(2), (ctypes.c_uint64 * 3)()
    assert zg.lib().zg_blocks_verify(ctx._p, 2, arena, off, 1, 1, 0, st, None, None, None, cnt, None) == -1
    assert zg.lib().zg_blocks_verify(ctx._p, 2, arena, None, 1, 1, 0, st, None, None, None, cnt, None) == -1


def test_ids_of_block_h522_feed_an_unrelated_entry(ctx):
    """the returned ids as prevouts' transactions: the block's transactions go through zg_sighash, which still
    succeeds, and a second blocks_verify returns the same ids"""
    raw = dict((n, r) for n, r, _ in C.fixtures())["block_h522"]
    ids = verify(ctx, [raw])[5][0]
    off = R.layout(raw)[2]
    txs = [raw[a:b] for a, b in zip(off, off[1:])]
    assert ids == want_ids(txs) and len(ids) == 9
    from tests import sighash_ref as S
    items = [(t, 0, b"\x76\xa9", 0, 1) for t in range(1, len(txs))]
    ts, hs, st = ctx.sighash(txs, [0] * len(txs), items)
    assert ts == [0] * 9 and st == [0] * 8
    assert hs == [S.sighash(txs[t], 0, b"\x76\xa9", 0, 1, 0)[0] for t in range(1, 9)]
    assert verify(ctx, [raw])[5][0] == ids


def test_kernel_time_covers_the_call(ctx):
    verify(ctx, [C.synthetic(5)])
    assert ctx.last_sig_kernel_ms() > 0


def test_writer_with_and_without_raw(ctx):
    from zebra_amd.blocks_writer import Block, DeferredBlocksWriter, MemoryStorage, WriterError
    g = b"g" * 32
    raws = [C.synthetic(2, seed=s) for s in range(3)]
    hashes = [R.dhash256(r[:R.HEADER_BYTES]) for r in raws]

    def chain(raw_of, header_of=lambda k: None):
        return [Block(hashes[k], g if k == 0 else hashes[k - 1], [], raw=raw_of(k), header=header_of(k))
                for k in range(3)]

    def run(blocks, **kw):
        st = MemoryStorage(g)
        w = DeferredBlocksWriter(st, ctx=ctx, verify_window=lambda txs: None, **kw)
        err = None
        try:
            for b in blocks:
                w.append_block(b)
            w.flush()
        except WriterError as e:
            err = e
        return st.blocks[1:], err, w

    calls = []
    stored, err, w = run(chain(lambda k: None), verify_blocks=lambda raws: calls.append(raws))
    assert (stored, err, calls, w.txids) == (hashes, None, [], {})      # raw=None: nothing changes, no call
    stored, err, w = run(chain(lambda k: raws[k]))
    assert (stored, err) == (hashes, None)
    assert w.txids == {hashes[k]: R.verify(raws[k], C.BIG, C.BIG)[4] for k in range(3)}
    bad = bytearray(raws[1])
    bad[40] ^= 1
    stored, err, w = run(chain(lambda k: bytes(bad) if k == 1 else raws[k]))
    assert stored == hashes[:1] and err == WriterError("Verification", "MerkleRoot") and list(w.txids) == hashes[:1]
    # a block-body error outranks the same block's header error; an earlier block's header error outranks it
    hdr_fail = lambda at: (lambda headers: [3 if k == at else 0 for k in range(len(headers))])
    hdr = lambda k: raws[k][:R.HEADER_BYTES]
    stored, err, _ = run(chain(lambda k: bytes(bad) if k == 1 else raws[k], hdr), verify_headers=hdr_fail(1))
    assert stored == hashes[:1] and err == WriterError("Verification", "MerkleRoot")
    stored, err, _ = run(chain(lambda k: bytes(bad) if k == 1 else raws[k], hdr), verify_headers=hdr_fail(0))
    assert stored == [] and err == WriterError("Verification", "Pow")
    # the detail word reaches the error: Error::Size(size)
    stored, err, _ = run(chain(lambda k: raws[k]), max_block_size=len(raws[0]) - 1)
    assert stored == [] and err == WriterError("Verification", ("Size", len(raws[0])))
