#!/usr/bin/env python3
"""Generate tests/golden/equihash.json: the fixtures of the block-header checks (Equihash solution,
proof of work, block hash). Hex data only.

Reads the reference as TEXT only (test-data/src/lib.rs: the 13 real blocks, first 1487 bytes each;
verification/src/equihash.rs:403-411: the (96, 5) test vector). Every expected verdict comes from
tests/equihash_ref.py. Asserted before anything is written: all 13 real headers have a valid
solution and valid proof of work against mainnet's limit (the reference's own block_h170 test among
them), the (96, 5) vector verifies, every named (200, 9) mutant is rejected, and the crafted (48, 5)
solutions are all accepted by the restatement while strict_distinct rejects exactly the
repeated-index ones.

    python tests/golden/gen_equihash.py [path to the reference checkout]
"""
import json
import os
import re
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import equihash_ref as Q  # noqa: E402

HEIGHTS = [0, 1, 2, 3, 9, 169, 170, 181, 182, 522, 567, 1033, 419221]
REF96_INPUT = b"Equihash is an asymmetric PoW based on the Generalised Birthday problem."
REF96_INDICES = [2261, 15185, 36112, 104243, 23779, 118390, 118332, 130041, 32642, 69878, 76925, 80080, 45858,
                 116805, 92842, 111026, 15972, 115059, 85191, 90330, 68190, 122819, 81830, 91132, 23460, 49807,
                 52426, 80391, 69567, 114474, 104973, 122568]
QUIRK_PREFIX = b"zg equihash quirk search"


def real_headers(ref):
    src = open(os.path.join(ref, "test-data", "src", "lib.rs")).read()
    out = []
    for h in HEIGHTS:
        # block_h419221 is the block of block_h419221_with_donors (test-data/src/lib.rs:117-131)
        m = re.search(r'pub fn block_h%d(?:_with_donors)?\(\) -> [^{]*\{\s*\(?\s*"([0-9a-f]+)"' % h, src)
        out.append((h, bytes.fromhex(m.group(1))[:Q.HEADER_BYTES]))
    return out


def swap_subtrees(idx, level, pair=0):
    """the two sibling subtrees of 2^level leaves under pair `pair` of that level, exchanged"""
    w = 1 << level
    o = pair * 2 * w
    return idx[:o] + idx[o + w:o + 2 * w] + idx[o:o + w] + idx[o + 2 * w:]


def with_indices(header, idx):
    return header[:143] + Q.compress_indices(Q.Params(200, 9), idx)


def mutants(headers):
    P = Q.Params(200, 9)
    by_h = dict(headers)
    out = []
    for level in range(9):
        base = HEIGHTS[level]
        hd = by_h[base]
        out.append(("swap_level_%d" % level, base, with_indices(hd, swap_subtrees(Q.solution_indices(P, hd[143:]), level,
                                                                                   pair=level % (256 >> level)))))
    hd = by_h[170]
    idx = Q.solution_indices(P, hd[143:])
    out.append(("index_xor_1", 170, with_indices(hd, idx[:5] + [idx[5] ^ 1] + idx[6:])))
    out.append(("leaf1_equals_leaf0", 170, with_indices(hd, [idx[0], idx[0]] + idx[2:])))
    out.append(("nonce_bit", 170, hd[:108] + bytes([hd[108] ^ 1]) + hd[109:]))
    out.append(("solution_bit", 170, hd[:843] + bytes([hd[843] ^ 0x10]) + hd[844:]))
    out.append(("solution_last_bit", 419221, by_h[419221][:-1] + bytes([by_h[419221][-1] ^ 1])))
    out.append(("bad_solution_length", 170, hd[:141] + b"\x41" + hd[142:]))
    return out


# ------------------------------------------------------------------ relaxed Wagner search
def wagner(n, k, data, relaxed=True):
    """every solution the reference accepts that a pairwise collision search finds: collide on each
    chunk, order left before right by first index, and (relaxed) check only the left row's first
    index against the right row, as distinct_indices does. -> list of index lists"""
    p = Q.Params(n, k)
    cb = p.BSTR_INDEX_BITS
    rows = []
    hashes = {}
    for i in range(1 << (cb + 1)):
        g = i // p.BSTRS_PER_HASH
        if g not in hashes:
            hashes[g] = Q.generate_hash(p, data, g)
        o = (i % p.BSTRS_PER_HASH) * n // 8
        rows.append((int.from_bytes(hashes[g][o:o + n // 8], "big"), (i,)))
    bits = n
    for level in range(k):
        bits -= cb
        last = level == k - 1
        buckets = {}
        for v, idx in rows:
            buckets.setdefault(v >> bits if not last else v, []).append((v, idx))
        nxt = []
        for group in buckets.values():
            for a in range(len(group)):
                for b in range(a + 1, len(group)):
                    (va, ia), (vb, ib) = group[a], group[b]
                    if ia[0] > ib[0]:
                        ia, ib = ib, ia
                    if ia[0] in ib if relaxed else set(ia) & set(ib):
                        continue
                    x = (va ^ vb) & ((1 << bits) - 1)
                    if not last and x == 0:
                        continue            # the rest cancels already: the same leaves twice
                    nxt.append((x, ia + ib))
        rows = nxt
    return [list(idx) for _, idx in rows]


def quirk_input(nonce, length=56):
    pre = QUIRK_PREFIX + bytes(range(length - 32 - len(QUIRK_PREFIX)))
    return pre + nonce.to_bytes(32, "little")


def crafted(length, want_ordinary, want_repeated, max_nonce=64):
    """every solution found over nonces 0, 1, ... until both counts are reached"""
    p = Q.Params(48, 5)
    out = []
    for nonce in range(max_nonce):
        data = quirk_input(nonce, length)
        for idx in wagner(48, 5, data):
            sol = Q.compress_indices(p, idx)
            rep = len(set(idx)) != len(idx)
            assert Q.verify(48, 5, data, sol)
            assert Q.strict_distinct(48, 5, sol) == (not rep)
            out.append({"input": data.hex(), "solution": sol.hex(), "repeated": int(rep)})
        nr = sum(e["repeated"] for e in out)
        if len(out) - nr >= want_ordinary and nr >= want_repeated:
            return out
    raise AssertionError("search found too few solutions: %r" % [e["repeated"] for e in out])


def pow_vectors(headers):
    T = Q.compact_to_u256
    vec = []

    def add(name, max_bits, bits, value):
        h = (value & ((1 << 256) - 1)).to_bytes(32, "little")
        vec.append({"name": name, "max_bits": max_bits, "bits": bits, "hash": h.hex(),
                    "valid": int(Q.is_valid_proof_of_work(max_bits, bits, h))})

    big = 0x2100ffff            # 0xffff << 240: the largest compact without overflow
    for bits, name in ((0x01003456, "size1_zero"), (0x01123456, "size1"), (0x02008000, "size2"),
                       (0x03123456, "size3"), (0x00123456, "size0"), (0x02123456, "size2_word")):
        t = T(bits)[1]
        add(name + "_eq", big, bits, t)
        add(name + "_above", big, bits, t + 1)
    # the sign bit: with a zero word it is no error; size <= 3 shifts the word first
    add("sign_zero_word", big, 0x04800000, 0)
    add("sign_nonzero_word", big, 0x04923456, 0)
    add("sign_size1_word_shifted_out", big, 0x01803456, 0)     # word >> 16 == 0x00: not negative
    add("sign_size2_word_kept", big, 0x02803456, 0)            # word >> 8 == 0x34: negative
    add("sign_as_max_bits", 0x04923456, 0x03000001, 0)
    # the three overflow clauses, each at its edge
    add("overflow_size35", big, 0x23000001, 0)
    add("size34_byte_ok", big, 0x220000ff, 0)
    add("overflow_size34_word", big, 0x22000100, 0)
    add("size33_two_bytes_ok", big, 0x2100ffff, 0)
    add("overflow_size33_word", big, 0x21010000, 0)
    add("overflow_as_max_bits", 0x23000001, 0x1f07ffff, 0)
    # hash against target
    t = T(0x1f07ffff)[1]
    add("hash_eq_target", 0x1f07ffff, 0x1f07ffff, t)
    add("hash_target_minus_1", 0x1f07ffff, 0x1f07ffff, t - 1)
    add("hash_target_plus_1", 0x1f07ffff, 0x1f07ffff, t + 1)
    add("hash_top_word_only", 0x1f07ffff, 0x1f07ffff, 1 << 255)
    add("target_above_max", 0x1f07fffe, 0x1f07ffff, 0)
    add("target_eq_max", 0x1f07ffff, 0x1f07ffff, 0)
    add("target_above_max_size", 0x1f07ffff, 0x2007ffff, 0)
    for h, hd in headers[:3]:
        bits = struct.unpack_from("<I", hd, 104)[0]
        add("real_h%d" % h, Q.MAINNET_MAX_BITS, bits, int.from_bytes(Q.block_hash(hd), "little"))
    assert {v["valid"] for v in vec} == {0, 1}
    return vec


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ZG_REFERENCE", os.path.join(ROOT, "..", "reference"))
    headers = real_headers(ref)
    real = []
    for h, hd in headers:
        f, hh = Q.header_flags(hd, Q.MAINNET_MAX_BITS)
        assert f == 0 and Q.header_status(hd, Q.MAINNET_MAX_BITS) == Q.HDR_OK, h
        real.append({"height": h, "header": hd.hex(), "hash": hh.hex()})
    assert real[0]["hash"][-8:] == "e80f0400" and real[1]["hash"][-8:] == "22bc0700"   # 00040fe8..., 0007bc22...
    assert Q.verify(200, 9, dict(headers)[170][:140], dict(headers)[170][143:])          # test_equihash_on_real_block

    p96 = Q.Params(96, 5)
    in96 = REF96_INPUT + (1).to_bytes(32, "little")
    sol96 = Q.compress_indices(p96, REF96_INDICES)
    assert Q.verify(96, 5, in96, sol96)
    ref96 = {"input": in96.hex(), "solution": sol96.hex(), "ok": 1, "swaps": []}
    for level in range(5):
        s = Q.compress_indices(p96, swap_subtrees(REF96_INDICES, level, pair=level % (16 >> level)))
        assert not Q.verify(96, 5, in96, s)
        ref96["swaps"].append({"level": level, "solution": s.hex(), "ok": 0})

    muts = []
    for name, base, hd in mutants(headers):
        f, hh = Q.header_flags(hd, Q.MAINNET_MAX_BITS)
        st = Q.header_status(hd, Q.MAINNET_MAX_BITS)
        assert st != Q.HDR_OK, name
        muts.append({"name": name, "base": base, "header": hd.hex(), "hash": hh.hex(), "status": st, "flags": f})
    got = {m["name"]: (m["status"], m["flags"]) for m in muts}
    assert got["nonce_bit"] == (Q.HDR_EQUIHASH, Q.F_EQUIHASH | Q.F_POW)
    assert got["leaf1_equals_leaf0"][1] & Q.F_REPEATED and not got["index_xor_1"][1] & Q.F_REPEATED
    assert got["bad_solution_length"][0] == Q.HDR_MALFORMED
    # (a changed solution changes the block hash too, so most mutants also fail the proof of work)
    assert all(st == Q.HDR_EQUIHASH and f & Q.F_EQUIHASH for n, (st, f) in got.items() if n != "bad_solution_length")

    c48 = crafted(56, 4, 3)
    assert sum(e["repeated"] for e in c48) >= 3 and sum(1 - e["repeated"] for e in c48) >= 4
    boundary = [[e for e in crafted(n, 1, 0) if not e["repeated"]][0] for n in (128, 129)]
    assert [len(e["input"]) // 2 for e in boundary] == [128, 129]

    out = {"max_bits": Q.MAINNET_MAX_BITS, "real": real, "ref96": ref96, "mutants": muts, "crafted48": c48,
           "boundary48": boundary, "pow": pow_vectors(headers)}
    path = os.path.join(HERE, "equihash.json")
    json.dump(out, open(path, "w"), indent=0)
    print("wrote %s: %d real, %d mutants, %d crafted (%d repeated), %d pow vectors, %d bytes" %
          (path, len(real), len(muts), len(c48), sum(e["repeated"] for e in c48), len(out["pow"]),
           os.path.getsize(path)))


if __name__ == "__main__":
    main()
