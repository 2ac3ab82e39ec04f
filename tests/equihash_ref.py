"""Byte-level restatement of the reference's block-header checks, the oracle of zg_equihash_verify /
zg_headers_verify / zg_pow_valid.

  verify(n, k, input, solution)   verify_equihash_solution (verification/src/equihash.rs:80-172): rows
        as padded byte strings, the same helpers expand_array / has_collision / indices_before /
        distinct_indices / merge_rows, BLAKE2b from hashlib with the "ZcashPoW" || LE32(N) || LE32(K)
        personalization. distinct_indices is restated AS WRITTEN (equihash.rs:258-274): `j` is not
        reset, so only the FIRST index of the left row is compared with the right row's indices. The
        reference therefore accepts some solutions with a repeated index that the Zcash specification
        rejects; strict_distinct() is the specification's rule, for telling those apart.
  compact_to_u256 / is_valid_proof_of_work   primitives/src/compact.rs:45-66 and
        verification/src/work.rs:21-34 as written (`word` is shifted BEFORE the sign and overflow tests
        when size <= 3).
  header_status / header_flags / block_hash   HeaderEquihashSolution::check then HeaderProofOfWork::check
        (verify_header.rs:48-54,116-124) over the 1487 serialized header bytes.

Nothing here is fast: a (200, 9) check takes a few milliseconds of Python."""
import hashlib
import struct

HEADER_BYTES = 1487
HDR_OK, HDR_MALFORMED, HDR_EQUIHASH, HDR_POW = 0, 1, 2, 3
F_EQUIHASH, F_POW, F_REPEATED = 1, 2, 4
MAINNET_MAX_BITS = 0x1f07ffff   # network/src/network.rs: Network::Mainnet max_bits, as a compact


class Params:
    """the associated constants of `trait Equihash` (equihash.rs:31-62)"""

    def __init__(self, n, k):
        self.N, self.K = n, k
        self.PERSONAL = b"ZcashPoW" + struct.pack("<II", n, k)
        self.BSTRS_PER_HASH = 512 // n
        self.HASH_SIZE = self.BSTRS_PER_HASH * n // 8
        self.BSTR_INDEX_BITS = n // (k + 1)
        self.BSTR_INDEX_BYTES = (self.BSTR_INDEX_BITS + 7) // 8
        self.BSTR_INDICES_IN_SOLUTION = 1 << k
        self.SOLUTION_COMPRESSED_SIZE = self.BSTR_INDICES_IN_SOLUTION * (self.BSTR_INDEX_BITS + 1) // 8
        self.SOLUTION_PAD_BYTES = 4 - (self.BSTR_INDEX_BITS + 8) // 8
        self.ROW_SIZE = 2 * self.BSTR_INDEX_BYTES + 4 * self.BSTR_INDICES_IN_SOLUTION
        self.ROW_HASH_LENGTH = (k + 1) * self.BSTR_INDEX_BYTES


def expand_array(compressed, blen, pad):
    """equihash.rs:194-230 -> list of 4-byte buffers (the buffer is reused there: bytes below `pad`
    stay zero)"""
    out_width = (blen + 7) // 8 + pad
    blen_mask = (1 << blen) - 1
    out = []
    acc_buffer = bytearray(4)
    acc_bits = 0
    acc_value = 0
    for c in compressed:
        acc_value = ((acc_value << 8) | c) & 0xFFFFFFFF
        acc_bits += 8
        if acc_bits >= blen:
            acc_bits -= blen
            for x in range(pad, out_width):
                acc_buffer[x] = ((acc_value >> (acc_bits + 8 * (out_width - x - 1))) & 0xFF) & \
                    ((blen_mask >> (8 * (out_width - x - 1))) & 0xFF)
            out.append(bytes(acc_buffer))
    return out


def solution_indices(p, solution):
    """for_each_solution_index (equihash.rs:174-192)"""
    assert len(solution) == p.SOLUTION_COMPRESSED_SIZE
    return [int.from_bytes(b, "big") for b in expand_array(solution, p.BSTR_INDEX_BITS + 1, p.SOLUTION_PAD_BYTES)]


def compress_indices(p, indices):
    """get_minimal_from_indices (equihash.rs:348-361): the big-endian bit stream of the indices"""
    bits = p.BSTR_INDEX_BITS + 1
    v = 0
    for i in indices:
        assert 0 <= i < (1 << bits)
        v = (v << bits) | i
    return v.to_bytes(len(indices) * bits // 8, "big")


def generate_hash(p, data, index):
    """generate_hash (equihash.rs:232-236) on the context of equihash.rs:85-86"""
    return hashlib.blake2b(data + struct.pack("<I", index), digest_size=p.HASH_SIZE, person=p.PERSONAL).digest()


def has_collision(row1, row2, n):
    for i in range(n):
        if row1[i] != row2[i]:
            return False
    return True


def indices_before(row1, row2, length, indices_len):
    for i in range(indices_len):
        if row1[length + i] < row2[length + i]:
            return True
        elif row1[length + i] > row2[length + i]:
            return False
    return False


def distinct_indices(row1, row2, length, indices_len):
    """as written: j is never reset, so the inner loop runs once, for i = 0"""
    i = 0
    j = 0
    while i < indices_len:
        while j < indices_len:
            if row1[length + i:length + i + 4] == row2[length + j:length + j + 4]:
                return False
            j += 4
        i += 4
    return True


def merge_rows(row1, row2, merged, length, indices_len, trim):
    pos = 0
    for i in range(trim, length):
        merged[pos] = row1[i] ^ row2[i]
        pos += 1
    a, b = (row1, row2) if indices_before(row1, row2, length, indices_len) else (row2, row1)
    merged[length - trim:length - trim + indices_len] = a[length:length + indices_len]
    merged[length - trim + indices_len:length - trim + 2 * indices_len] = b[length:length + indices_len]


def initial_rows(p, data, solution):
    rows = []
    for index in solution_indices(p, solution):
        h = generate_hash(p, data, index // p.BSTRS_PER_HASH)
        begin = (index % p.BSTRS_PER_HASH) * p.N // 8
        sub = h[begin:begin + p.N // 8]
        row = bytearray(p.ROW_SIZE)
        pos = 0
        for buf in expand_array(sub, p.BSTR_INDEX_BITS, 0):
            row[pos:pos + p.BSTR_INDEX_BYTES] = buf[:p.BSTR_INDEX_BYTES]
            pos += p.BSTR_INDEX_BYTES
        row[p.ROW_HASH_LENGTH:p.ROW_HASH_LENGTH + 4] = index.to_bytes(4, "big")
        rows.append(row)
    return rows


def verify(n, k, data, solution):
    """verify_equihash_solution::<(n, k)>(data, solution)"""
    p = Params(n, k)
    rows = initial_rows(p, data, solution)
    hash_len = p.ROW_HASH_LENGTH
    indices_len = 4
    while len(rows) > 1:
        nxt = []
        for i in range(len(rows) // 2):
            row1, row2 = rows[2 * i], rows[2 * i + 1]
            if not has_collision(row1, row2, p.BSTR_INDEX_BYTES):
                return False
            if indices_before(row2, row1, hash_len, indices_len):
                return False
            if not distinct_indices(row1, row2, hash_len, indices_len):
                return False
            merged = bytearray(p.ROW_SIZE)
            merge_rows(row1, row2, merged, hash_len, indices_len, p.BSTR_INDEX_BYTES)
            nxt.append(merged)
        rows = nxt
        hash_len -= p.BSTR_INDEX_BYTES
        indices_len *= 2
    return all(x == 0 for x in rows[0][:hash_len])


def strict_distinct(n, k, solution):
    """the specification's rule: all 2^k indices differ"""
    idx = solution_indices(Params(n, k), solution)
    return len(set(idx)) == len(idx)


# ------------------------------------------------------------------ proof of work
def compact_to_u256(c):
    """Compact::to_u256 (compact.rs:45-66) -> (ok, value)"""
    size = c >> 24
    word = c & 0x007fffff
    if size <= 3:
        word >>= 8 * (3 - size)
        result = word
    else:
        result = (word << (8 * (size - 3))) & ((1 << 256) - 1)
    is_negative = word != 0 and (c & 0x00800000) != 0
    is_overflow = (word != 0 and size > 34) or (word > 0xff and size > 33) or (word > 0xffff and size > 32)
    return (not (is_negative or is_overflow)), result


def is_valid_proof_of_work(max_bits, bits, hash32):
    """work.rs:21-34; hash32 in H256 storage order (value = the reversed bytes, big-endian)"""
    ok, maximum = compact_to_u256(max_bits)
    if not ok:
        return False
    ok, target = compact_to_u256(bits)
    if not ok:
        return False
    value = int.from_bytes(hash32, "little")
    return target <= maximum and value <= target


# ------------------------------------------------------------------ headers
def block_hash(header):
    """BlockHeader::hash (chain/src/block_header.rs:64-66): dhash256 of the serialized header, in
    H256 storage order"""
    return hashlib.sha256(hashlib.sha256(header).digest()).digest()


def header_flags(header, max_bits):
    """every check on its own, over bytes 143.. whatever bytes 140..142 say -> (F_* mask, hash)"""
    assert len(header) == HEADER_BYTES
    hh = block_hash(header)
    sol = header[143:]
    bits = struct.unpack_from("<I", header, 104)[0]
    f = 0
    if not verify(200, 9, header[:140], sol):
        f |= F_EQUIHASH
    if not is_valid_proof_of_work(max_bits, bits, hh):
        f |= F_POW
    if not strict_distinct(200, 9, sol):
        f |= F_REPEATED
    return f, hh


def header_status(header, max_bits):
    """the first failing check in the reference's order: EquihashSolution::deserialize (the compact
    size 1344 = fd 40 05), HeaderEquihashSolution::check, HeaderProofOfWork::check"""
    if header[140:143] != b"\xfd\x40\x05":
        return HDR_MALFORMED
    f = header_flags(header, max_bits)[0]
    if f & F_EQUIHASH:
        return HDR_EQUIHASH
    if f & F_POW:
        return HDR_POW
    return HDR_OK
