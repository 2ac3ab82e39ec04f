"""CPU tier of the block body checks: the restatement tests/blocks_ref.py, the library's host
parser zg_block_layout, and a host build of the routines the kernels run (tests/blocks_hostlib.py), against the
fixtures of tests/golden/blocks.json and synthetic blocks. The GPU tier is tests/test_gpu_blocks.py."""
import hashlib
import shutil
import subprocess

import pytest

from tests import blocks_cases as C
from tests import blocks_ref as R
from tests.conftest import load_golden
from zebra_amd import zg

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def test_restatement_matches_every_fixture():
    g = load_golden("blocks.json")
    assert [e["layout"][0] for e in g["blocks"] if e["name"] in ("block_h567", "block_h522")] == [2, 9]
    for e in g["blocks"]:
        raw = bytes.fromhex(e["raw"])
        st, flags, _, root, ids = R.verify(raw, C.BIG, C.BIG)
        assert (st, flags) == (R.BLK_OK, 0), e["name"]
        assert root.hex() == e["merkle_root"] == raw[36:68].hex() and [i.hex() for i in ids] == e["txids"]
    for m in g["merkle"]:
        assert R.merkle_root([bytes.fromhex(x) for x in m["leaves"]]).hex() == m["root"]


def test_layout_of_every_fixture_block():
    for name, raw, e in C.fixtures():
        st, out, off = zg.block_layout(raw)
        assert (st, out, off) == (zg.TX_OK, e["layout"], e["tx_off"]) == R.layout(raw), name
        assert out[1] == out[5] == len(raw) and out[3] == 1 and out[4] == zg.BLK_NO_INDEX


def test_offsets_are_written_only_when_the_capacity_suffices():
    import ctypes
    raw = dict((n, r) for n, r, _ in C.fixtures())["block_h522"]
    out = (ctypes.c_uint64 * 6)()
    buf = (ctypes.c_uint64 * 10)(*[7] * 10)
    assert zg.lib().zg_block_layout(raw, len(raw), out, buf, 9) == zg.TX_OK and out[0] == 9 and list(buf) == [7] * 10
    assert zg.lib().zg_block_layout(raw, len(raw), out, buf, 10) == zg.TX_OK and buf[0] == 1488 and buf[9] == len(raw)


def test_every_proper_prefix_is_malformed():
    blocks = dict((n, r) for n, r, _ in C.fixtures())
    for raw in (blocks["block_parse_1"], C.synthetic(3)):
        assert zg.block_layout(raw)[0] == zg.TX_OK
        for k in range(len(raw)):
            assert zg.block_layout(raw[:k]) == (zg.TX_MALFORMED, [0] * 6, None), k


def test_trailing_bytes_and_bad_solution_prefix_are_malformed():
    raw = C.synthetic(2)
    assert zg.block_layout(raw + b"\x00")[0] == zg.TX_MALFORMED
    for at, byte in ((140, 0xFC), (141, 0x41), (142, 0x04)):
        bad = bytearray(raw)
        bad[at] = byte
        assert zg.block_layout(bytes(bad))[0] == R.layout(bytes(bad))[0] == zg.TX_MALFORMED


def test_transaction_count_edges():
    hdr = C.header()
    empty = hdr + b"\x00"
    assert zg.block_layout(empty) == (zg.TX_OK, [0, 1488, 0, 0, zg.BLK_NO_INDEX, 1488], [1488]) == R.layout(empty)
    big = hdr + b"\xff" + (1 << 32).to_bytes(8, "little")
    assert zg.block_layout(big)[0] == R.layout(big)[0] == zg.TX_MALFORMED
    good = C.synthetic(3)
    for form in (0xFD, 0xFE, 0xFF):
        nc = C.noncanonical_count(good, form)
        st, out, off = zg.block_layout(nc)
        assert (st, out, off) == R.layout(nc) and st == zg.TX_NONCANONICAL
        assert out[0] == 3 and out[1] == len(good) and out[5] == len(nc)   # size: what the writer would emit


def test_a_noncanonical_transaction_inside_a_good_block():
    txs = [R.min_tx(0, coinbase=True), R.min_tx(1), R.min_tx(2)]
    t = txs[1]
    assert t[4] == 1
    txs[1] = t[:4] + b"\xfd\x01\x00" + t[5:]     # its input count in the three-byte form
    raw = R.make_block(C.header(), txs)
    st, out, off = zg.block_layout(raw)
    assert st == zg.TX_NONCANONICAL and (st, out, off) == R.layout(raw) and out[1] == len(raw) - 2


def test_fixture_sigops_scripts():
    for e in load_golden("blocks.json")["sigops"]:
        script = R.script_from_recipe(e)
        assert R.script_sigops(script) == e["count"]
        raw = R.make_block(C.header(), [R.min_tx(0, coinbase=True), R.min_tx(1, out_script=script)])
        assert zg.block_layout(raw)[1][2] == e["count"], e["count"]


def test_sigops_edges():
    def sigops(**kw):
        raw = R.make_block(C.header(), [R.min_tx(0, coinbase=True, **kw.pop("cb", {})), R.min_tx(1, **kw)])
        st, out, _ = zg.block_layout(raw)
        assert st == zg.TX_OK and out == R.layout(raw)[1]
        return out[2]
    assert sigops(out_script=b"\xac\xad\xae\xaf") == 42
    assert sigops(out_script=b"\xac\x05\xac\xac") == 1            # a truncated push: the count so far
    assert sigops(out_script=b"\xac\x4c\x03\xac\xac") == 1        # PUSHDATA1 past the end
    assert sigops(out_script=b"\xac\x4d\x01") == 1                # PUSHDATA2 without its length
    assert sigops(out_script=b"\xac\x4e\xff\xff\xff\xff\xac") == 1
    assert sigops(out_script=b"\x02\xac\xac\xac") == 1            # pushed bytes are not opcodes
    assert sigops(out_script=b"\xac\xab\xac") == 1                # 0xab: not in Opcode::from_u8
    assert sigops(out_script=b"\xac\xba\xac") == 1 and sigops(out_script=b"\xac\xff\xac") == 1
    assert sigops(out_script=b"\xac\xb9\xac") == 2                # OP_NOP10 is the last known
    assert sigops(in_script=b"\xac\xac") == 2                     # input scripts count ...
    assert sigops(cb={"in_script": b"\xac\xac\xac"}) == 0         # ... but not a coinbase's
    assert sigops(cb={"out_script": b"\xae"}) == 20               # its outputs do


def test_failing_checks_alone_and_in_pairs_in_the_restatement():
    """the synthetic blocks fail exactly what they were built to fail, and the first in the reference's order
    is the status; the library's parser agrees with the restatement on what the host decides"""
    order = [R.F_EMPTY, R.F_COINBASE, R.F_SIZE, R.F_EXTRA_COINBASE, R.F_DUPLICATED, R.F_SIGOPS, R.F_MERKLE_ROOT]
    for name, (raw, max_size, max_sigops, flags) in C.failing_cases():
        st, got, detail, _, _ = R.verify(raw, max_size, max_sigops)
        assert got == flags, name
        assert st == (R.BLK_EMPTY + order.index(next(f for f in order if f & flags)) if flags else R.BLK_OK), name
        assert detail == (len(raw) if st == R.BLK_SIZE else 3 if st == R.BLK_EXTRA_COINBASE else 0), name
        assert zg.block_layout(raw) == R.layout(raw), name


@needs_hipcc
def test_host_build_matches_every_fixture():
    from tests import blocks_hostlib as H
    g = load_golden("blocks.json")
    for name, raw, e in C.fixtures():
        st, out, off = H.block_layout(raw)
        assert (st, out, off) == (0, e["layout"], e["tx_off"]), name
        ids = H.txids([raw[a:b] for a, b in zip(off, off[1:])], threads=3)
        assert [i.hex() for i in ids] == e["txids"], name
        assert H.merkle_root(ids).hex() == e["merkle_root"], name
    for m in g["merkle"]:
        assert H.merkle_root([bytes.fromhex(x) for x in m["leaves"]]).hex() == m["root"]


@needs_hipcc
def test_host_build_reader_at_every_length_and_alignment():
    from tests import blocks_hostlib as H
    data = hashlib.shake_128(b"zg blocks").digest(4096)
    slices = [data[7:7 + n] for n in range(201)]
    assert H.txids(slices) == [R.dhash256(s) for s in slices]
    # one arena, slices back to back: every start alignment mod 16 comes up for every padding edge
    slices = [data[k:k + n] for n in (0, 1, 15, 16, 17, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129) for k in range(16)]
    slices = [s + b"x" * k for k, s in enumerate(slices[:17])] + slices
    assert H.txids(slices, threads=4) == [R.dhash256(s) for s in slices]
    for k in (1, 2, 3, 4, 5, 16, 17, 255, 256, 257):
        ids = [hashlib.sha256(b"%d" % i).digest() for i in range(k)]
        assert H.merkle_root(ids) == R.merkle_root(ids), k


@needs_hipcc
def test_standalone_program_under_sanitizers(tmp_path):
    """parser and reader with their own main, address and undefined-behaviour sanitizers: every block and every
    proper prefix of two of them in heap blocks of exactly their size; the reader over arenas allocated exactly as
    the entry allocates them, each slice ending on the arena's last byte at every start alignment"""
    from tests import blocks_hostlib as H
    exe = H.build_program(str(tmp_path / "zg_hosttest_blocks"))
    lines, prefixes = [], 0
    for name, raw, e in C.fixtures():
        sweep = name in ("block_parse_0",)
        prefixes += len(raw) if sweep else 0
        lines.append("B %s 0 %s %d" % (raw.hex(), e["merkle_root"], int(sweep)))
    small = C.synthetic(5)
    prefixes += len(small)
    lines.append("B %s 0 %s 1" % (small.hex(), small[36:68].hex()))
    for name, (raw, _, _, _) in C.failing_cases():
        root = R.verify(raw, C.BIG, C.BIG)[3]
        lines.append("B %s 0 %s 0" % (raw.hex(), root.hex() if root else "-"))
    lines.append("B %s 1 - 0" % (small + b"\x00").hex())
    lines.append("B %s 2 - 0" % C.noncanonical_count(small, 0xFE).hex())
    lines.append("B %s 1 - 0" % (C.header() + b"\xff" + (1 << 32).to_bytes(8, "little")).hex())
    data = hashlib.shake_128(b"zg blocks").digest(300)
    lengths = list(range(0, 131)) + [191, 192, 193, 255, 256, 257]
    for n in lengths:
        lines.append("S %s %s" % (data[:n].hex() or "-", R.dhash256(data[:n]).hex()))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("cases %d mismatches 0 prefixes %d prefixes_parsed 0 slices %d"
                                     % (len(lines), prefixes, 16 * len(lengths))), p.stdout
