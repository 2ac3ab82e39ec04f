"""Block-header checks on the GPU: zg_headers_verify and zg_equihash_verify against
the fixture of tests/golden/equihash.json and the restatement tests/equihash_ref.py -- the 13 real
headers (status, hash, flags), the proof-of-work limit, every named (200, 9) mutant, batch shapes
over more than one workgroup wave, the (96, 5) and (48, 5) instances including the crafted solutions
on which the reference and the specification differ (ok = 1 with repeated = 1), solutions packed per
workgroup, inputs on both sides of the BLAKE2b block boundary, and the deferred writer through a
real context. The CPU tier is tests/test_equihash.py."""
import random

import pytest

from tests import equihash_ref as Q
from tests.test_equihash import fixture, h

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64, load_builtin=False)


def real_headers():
    return [h(e["header"]) for e in fixture()["real"]]


def test_real_headers(ctx):
    g = fixture()
    st, hashes, flags = ctx.headers_verify(real_headers(), g["max_bits"])
    assert st == [0] * 13 and flags == [0] * 13
    assert hashes == [h(e["hash"]) for e in g["real"]]
    assert ctx.headers_verify([], g["max_bits"]) == ([], [], [])


def test_max_bits_one_step_below_and_err_compact(ctx):
    from zebra_amd import zg
    g = fixture()
    hs = real_headers()
    for k in (0, 6, 12):
        bits = int.from_bytes(hs[k][104:108], "little")
        st, _, flags = ctx.headers_verify(hs, bits - 1)      # one step below this header's target
        for i, hd in enumerate(hs):
            want = Q.header_flags(hd, bits - 1)[0]
            assert flags[i] == want and st[i] == (zg.HDR_POW if want else 0), (k, i)
        assert st[k] == zg.HDR_POW and flags[k] == zg.HDR_F_POW
    for bad in (0x04923456, 0x23000001):                      # negative, overflow: Err -> Pow for all
        assert not Q.compact_to_u256(bad)[0]
        st, hashes, flags = ctx.headers_verify(hs, bad)
        assert st == [zg.HDR_POW] * 13 and flags == [zg.HDR_F_POW] * 13
        assert hashes == [h(e["hash"]) for e in g["real"]]


def test_mutants(ctx):
    from zebra_amd import zg
    g = fixture()
    ms = g["mutants"]
    st, hashes, flags = ctx.headers_verify([h(m["header"]) for m in ms], g["max_bits"])
    bad = [(m["name"], m["status"], m["flags"], s, f) for m, s, f in zip(ms, st, flags)
           if (s, f) != (m["status"], m["flags"])]
    assert not bad, bad
    assert hashes == [h(m["hash"]) for m in ms]
    got = {m["name"]: (s, f) for m, s, f in zip(ms, st, flags)}
    assert got["nonce_bit"] == (zg.HDR_EQUIHASH, zg.HDR_F_EQUIHASH | zg.HDR_F_POW)
    assert got["leaf1_equals_leaf0"][1] & zg.HDR_F_REPEATED


@pytest.mark.parametrize("n", [1, 2, 13, 65, 130])
def test_batch_shapes(ctx, n):
    g = fixture()
    real, ms = g["real"], g["mutants"]
    items = [real[i % 13] for i in range(n)]
    want = [(0, 0)] * n
    first, last = ms[n % len(ms)], ms[(n + 5) % len(ms)]
    items[-1], want[-1] = last, (last["status"], last["flags"])
    items[0], want[0] = first, (first["status"], first["flags"])
    st, hashes, flags = ctx.headers_verify([h(e["header"]) for e in items], g["max_bits"])
    assert list(zip(st, flags)) == want
    assert hashes == [h(e["hash"]) for e in items]


def test_equihash_200_9_direct(ctx):
    """zg_equihash_verify on the on-chain instance gives the Equihash flag of the header call"""
    from zebra_amd import zg
    g = fixture()
    items = g["real"][:3] + g["mutants"]
    hs = [h(e["header"]) for e in items]
    ok, rep = ctx.equihash_verify(zg.EQ_200_9, [x[:140] for x in hs], [x[143:] for x in hs])
    want = [0, 0, 0] + [m["flags"] for m in g["mutants"]]
    assert ok == [not f & Q.F_EQUIHASH for f in want]
    assert rep == [bool(f & Q.F_REPEATED) for f in want]


def test_reference_96_5_vector(ctx):
    from zebra_amd import zg
    r = fixture()["ref96"]
    sols = [h(r["solution"])] + [h(s["solution"]) for s in r["swaps"]]
    ok, rep = ctx.equihash_verify(zg.EQ_96_5, [h(r["input"])] * 6, sols)
    assert ok == [True] + [False] * 5 and rep == [False] * 6


def crafted():
    return [(h(e["input"]), h(e["solution"]), bool(e["repeated"])) for e in fixture()["crafted48"]]


def test_crafted_48_5_reference_verdict_and_repeated_flag(ctx):
    from zebra_amd import zg
    c = crafted()
    ok, rep = ctx.equihash_verify(zg.EQ_48_5, [x[0] for x in c], [x[1] for x in c])
    assert ok == [True] * len(c)                 # the reference's verdict, repeated index or not
    assert rep == [x[2] for x in c]              # ... and exactly the repeated ones flagged
    assert sum(rep) >= 3 and len(rep) - sum(rep) >= 4


def mutate48(sol, rnd):
    """a solution with two indices exchanged or one index changed (mostly rejects)"""
    p = Q.Params(48, 5)
    idx = Q.solution_indices(p, sol)
    how = rnd.randrange(3)
    if how == 0:
        i = rnd.randrange(31)
        idx[i], idx[i + 1] = idx[i + 1], idx[i]
    elif how == 1:
        idx[rnd.randrange(32)] ^= 1 << rnd.randrange(9)
    else:
        idx[rnd.randrange(32)] = idx[rnd.randrange(32)]
    return Q.compress_indices(p, idx)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 129])
def test_48_5_packing_and_wave_tail(ctx, n):
    """8 solutions per workgroup: sizes around the workgroup and the 64-item marks, a mix of accepted,
    repeated-index and mutated solutions, every verdict from the restatement"""
    from zebra_amd import zg
    c = crafted()
    rnd = random.Random(n)
    ins, sols = [], []
    for i in range(n):
        data, sol, _ = c[i % len(c)]
        if i % 3 == 1 and i != n - 1:
            sol = mutate48(sol, rnd)
        ins.append(data)
        sols.append(sol)
    ok, rep = ctx.equihash_verify(zg.EQ_48_5, ins, sols)
    assert ok == [Q.verify(48, 5, a, b) for a, b in zip(ins, sols)]
    assert rep == [not Q.strict_distinct(48, 5, b) for b in sols]
    assert ok[-1] and (n < 3 or not all(ok))


@pytest.mark.parametrize("length", [56, 104, 125, 127, 128, 129, 252])
def test_48_5_input_lengths(ctx, length):
    """one-block and two-block BLAKE2b, the index straddling the blocks (125, 127), an empty (128) and a
    full (252) final block; random inputs (rejects) plus, at 56 / 128 / 129 bytes, solved inputs"""
    from zebra_amd import zg
    g = fixture()
    rnd = random.Random(length)
    c = crafted()
    ins = [bytes(rnd.randrange(256) for _ in range(length)) for _ in range(9)]
    sols = [c[i % len(c)][1] for i in range(9)]
    solved = [(h(e["input"]), h(e["solution"])) for e in g["crafted48"] + g["boundary48"] if len(h(e["input"])) == length]
    assert bool(solved) == (length in (56, 128, 129))
    for a, b in solved:
        ins.append(a)
        sols.append(b)
    ok, rep = ctx.equihash_verify(zg.EQ_48_5, ins, sols)
    assert ok == [Q.verify(48, 5, a, b) for a, b in zip(ins, sols)]
    assert ok[9:] == [True] * len(solved)
    assert rep == [not Q.strict_distinct(48, 5, b) for b in sols]


def test_argument_checks(ctx):
    from zebra_amd import zg
    assert ctx.equihash_verify(zg.EQ_48_5, [], []) == ([], [])
    with pytest.raises(zg.ZgError):
        ctx.equihash_verify(zg.EQ_48_5, [b"\0" * 253], [b"\0" * 36])
    with pytest.raises(zg.ZgError):
        ctx.equihash_verify(zg.EQ_96_5, [b"\0" * 8], [b"\0" * 36])
    with pytest.raises(zg.ZgError):
        ctx.headers_verify([b"\0" * 1486], 0x1f07ffff)
    assert ctx.last_sig_kernel_ms() >= 0.0


def test_writer_with_real_context(ctx):
    """the consecutive real headers 169, 170 and 181, 182 with empty transaction lists and one mutant in
    the middle: the same blocks inserted and the same error raised as the fake backend predicts"""
    from zebra_amd.blocks_writer import Block, DeferredBlocksWriter, MemoryStorage, WriterError
    g = fixture()
    by_h = {e["height"]: h(e["header"]) for e in g["real"]}
    assert by_h[170][4:36] == Q.block_hash(by_h[169]) and by_h[182][4:36] == Q.block_hash(by_h[181])
    for name in (None, "swap_level_3", "nonce_bit", "leaf1_equals_leaf0", "bad_solution_length"):
        headers = [by_h[169], by_h[170], by_h[181], by_h[182]]
        if name is not None:
            headers.insert(2, h(next(m for m in g["mutants"] if m["name"] == name)["header"]))

        def blocks():
            return [Block(hash=i + 1, parent=i, txs=[], header=hd) for i, hd in enumerate(headers)]

        def run(**kw):
            st = MemoryStorage(0)
            w = DeferredBlocksWriter(st, **kw)
            err = None
            try:
                for b in blocks():
                    w.append_block(b)
                w.flush()
            except WriterError as e:
                err = (e.kind, e.detail)
            return st.blocks[1:], err

        fake = run(verify_window=lambda txs: None,
                   verify_headers=lambda hs: [Q.header_status(x, g["max_bits"]) for x in hs])
        real = run(ctx=ctx, max_bits=g["max_bits"])
        assert real == fake, name
        if name is None:
            assert real == ([1, 2, 3, 4], None)
        else:
            want = {"swap_level_3": "InvalidEquihashSolution", "nonce_bit": "InvalidEquihashSolution",
                    "leaf1_equals_leaf0": "InvalidEquihashSolution", "bad_solution_length": "MalformedHeader"}[name]
            assert real == ([1, 2], ("Verification", want)), name
    # a Pow error: the window against a limit below header 181's target
    bits = int.from_bytes(by_h[181][104:108], "little")
    st = MemoryStorage(0)
    w = DeferredBlocksWriter(st, ctx=ctx, max_bits=bits - 1)
    want_first = next(i for i, k in enumerate((169, 170, 181, 182)) if Q.header_status(by_h[k], bits - 1))
    with pytest.raises(WriterError) as ei:
        for i, k in enumerate((169, 170, 181, 182)):
            w.append_block(Block(hash=i + 1, parent=i, txs=[], header=by_h[k]))
        w.flush()
    assert ei.value.detail == "Pow" and st.blocks[1:] == list(range(1, want_first + 1))
