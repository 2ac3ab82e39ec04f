"""Case builders for the batch-path edge tests (tests/test_batch_edges.py on the CPU,
tests/test_gpu_batch_edges.py on the GPU): ragged sizes (n < npad), single-kind and two-kind mixes,
all fixture mutants in one batch, degenerate group sums forced by explicit batch scalars, extreme
scalar rows and input rows.

Every expectation here comes from the oracle alone: statuses and per-proof left-hand sides from the
C++ restatement of bellman's verify_proof (tests/cpulib.verify) or, for fixture items, from the
fixture's own `status` / `lhs_gt`; gt_out from oracle.groth16.batch_gt over the slots of status 0 or
3; partial bytes from oracle.groth16.batch_partial (affine_slots = npad where the affine R-chain
runs). Nothing here touches the GPU."""
import functools
import itertools
import random

from oracle import bls12_381 as B, groth16 as G
from tests import cpulib
from tests.conftest import load_golden

SRC_NAMES = ["S1", "S2", "O1", "O2", "O3", "J1", "J2", "J3", "J4"]
SIZES = [1, 2, 3, 5, 31, 33, 65, 129, 257]
PARTIAL_MAX, GT_MAX = 33, 129      # host time: the Python oracle's partial / gt_out up to these sizes
MIX_SIZES = [3, 33]
POOL = 257
VARIANTS = 4                       # re-randomisations per source (Python G2 arithmetic on the host)
RERAND_SEED = 0xED6E5
K4_DEFAULT_MIN = 16384             # zebra_amd/csrc/zg_host.h ZG_K4_MIN
MAX_BATCH = 512


# ------------------------------------------------------------------ schedules
def _schedules():
    from tests import test_gpu_affine, test_gpu_csum
    mark = [m for m in test_gpu_csum.test_context_knobs_give_the_same_partial.pytestmark
            if m.name == "parametrize"][0]
    out = [dict(e) for e in mark.args[1]]
    out += [dict(test_gpu_affine.LINE_PROD, ZG_LINE_GROUP=32, **v) for v in test_gpu_affine.VARIANTS]
    out += [{"ZG_LINES_FCHAIN": 0}, {"ZG_LINES_FCHAIN": 1}, {}, {"ZG_K4_MIN": 1 << 30}]
    for e in out:   # a group of 2,048 never fits the sizes used here
        if e.get("ZG_LINE_GROUP") == 2048:
            e["ZG_LINE_GROUP"] = 128
    return out


SCHEDULES = _schedules()
# section 3 (all mutants in one batch): default, fused 0 and 1, quads with groups of 32, K4 forced
MUTANT_SCHEDULES = [{}, {"ZG_LINES_FCHAIN": 0}, {"ZG_LINES_FCHAIN": 1},
                    {"ZG_LINES_FCHAIN": 0, "ZG_FCHAIN_QUADS": 1, "ZG_LINE_GROUP": 32}, {"ZG_K4_MIN": 1}]


def sched_id(env):
    return ",".join("%s=%s" % kv for kv in env.items()) or "default"


def npad_of(n):
    p = 2
    while p < n:
        p <<= 1
    return p


def expected_path(env, npad):
    """the launch shape run_pipeline (zebra_amd/csrc/zg.hip) takes for a lone batch of npad <= 512 padded
    proofs on a context created under env, restated from its clamps: the fused launch excludes quads;
    quads need npad >= 4; group line products need quads and a group size <= npad; the affine R-chain
    needs line products; K4 from ZG_K4_MIN padded proofs"""
    assert npad <= MAX_BATCH   # both grids of a fused launch are resident at once at these sizes
    fused = env.get("ZG_LINES_FCHAIN", -1) != 0
    quads = not fused and npad >= 4 and env.get("ZG_FCHAIN_QUADS", -1) == 1
    g = env.get("ZG_LINE_GROUP", -1)
    if g != -1 and (g < 4 or g & (g - 1)):
        g = 0
    gsize = 0 if g < 0 or g > npad else g    # (auto: line products only from 32,768 proofs)
    lineprod = quads and gsize > 0
    affine = lineprod and bool(env.get("ZG_LINES_AFFINE_XL") or env.get("ZG_LINES_AFFINE") in (2, 4, 8))
    return {"fused": fused, "quads": quads, "lineprod": lineprod, "affine": affine,
            "k4": npad >= env.get("ZG_K4_MIN", K4_DEFAULT_MIN)}


def path_name(p):
    f = "fused" if p["fused"] else "affine+lineprod" if p["affine"] else "lineprod" if p["lineprod"] else \
        "quads" if p["quads"] else "pairs"
    return f + ("/k4" if p["k4"] else "/glv")


# ------------------------------------------------------------------ oracle plumbing
@functools.lru_cache(maxsize=None)
def cpu():
    return cpulib.load()


@functools.lru_cache(maxsize=None)
def pvks():
    import os
    return {k: G.prepare_verifying_key(G.load_vk_json(open(os.path.join(cpulib.ROOT, "zebra_amd", "res", f)).read()))
            for k, f in cpulib.VK_FILES.items()}


_pow_cache = {}


def _lhs_pow(lhs, r16):
    key = (lhs, r16)
    if key not in _pow_cache:
        _pow_cache[key] = G.batch_gt([B.f12_from_bytes(lhs)], [G.batch_r(r16)])
    return _pow_cache[key]


def pack_rows(rows):
    """per proof a list of 32-byte LE values -> n x 288 bytes (zebra_amd.pack_inputs, without the library)"""
    out = bytearray(288 * len(rows))
    for i, row in enumerate(rows):
        for j, x in enumerate(row):
            out[288 * i + 32 * j:288 * i + 32 * j + 32] = x
    return bytes(out)


class Case:
    """one batch: the buffers zg_verify_batch / zg_batch_begin take, and the oracle's expectations
    (computed on first use, then kept)"""

    def __init__(self, name, proofs, kinds, inputs, r, nin=None, statuses=None, lhs=None):
        self.name, self.n = name, len(kinds)
        assert len(proofs) == 192 * self.n and len(inputs) == 288 * self.n and len(r) == 16 * self.n
        assert nin is None or len(nin) == self.n
        self.proofs, self.kinds, self.inputs, self.r, self.nin = bytes(proofs), bytes(kinds), bytes(inputs), bytes(r), nin
        self.npad = npad_of(self.n)
        self._st, self._lhs = statuses, lhs     # fixture items: the fixture's own status / lhs_gt
        self._gt = None
        self._partial = {}

    def _verify(self):
        if self._st is None:
            self._st, self._lhs = cpulib.verify(cpu(), self.proofs, self.kinds, self.inputs, self.nin, threads=8,
                                                want_gt=True) if self.n else ([], [])

    @property
    def statuses(self):
        self._verify()
        return list(self._st)

    @property
    def live(self):
        """slots in gt_out and in the partial: decoded with canonical inputs and a well-formed key"""
        return [i for i, s in enumerate(self.statuses) if s in (0, 3)]

    def r16(self, i):
        return self.r[16 * i:16 * i + 16]

    def count(self, i):
        return self.nin[i] if self.nin is not None else G.KIND_NINPUTS[self.kinds[i]]

    def gt(self):
        """gt_out: oracle.groth16.batch_gt over the live slots' oracle left-hand sides and batch_r of their
        scalar rows -- as the product of one-slot batch_gt values, each formed once per (LHS, r) and
        shared by every case that holds that slot"""
        if self._gt is None:
            self._verify()
            acc = B.F12_ONE
            for i in self.live:
                acc = B.f12_mul(acc, _lhs_pow(self._lhs[i], self.r16(i)))
            self._gt = B.f12_to_bytes(acc)
        return self._gt

    def items(self):
        """(kind, proof, inputs[:count], r) per slot, as oracle.groth16.batch_partial reads them"""
        out = []
        for i in range(self.n):
            row = self.inputs[288 * i:288 * i + 288]
            xs = [int.from_bytes(row[32 * j:32 * j + 32], "little") for j in range(self.count(i))]
            out.append((self.kinds[i], self.proofs[192 * i:192 * i + 192], xs, G.batch_r(self.r16(i))))
        return out

    def partial(self, affine=False):
        """the 576-byte Miller partial; affine: the affine R-chain's (every slot of npad without a live
        proof contributes the idle line's chain)"""
        if affine not in self._partial:
            self._partial[affine] = B.f12_to_bytes(
                G.batch_partial(pvks(), self.items(), affine_slots=self.npad if affine else None))
        return self._partial[affine]

    def c_terms(self, kind):
        """[(slot, r_i C_i)] of the live slots of one key, from the oracle's own decode"""
        out = []
        for i in self.live:
            if self.kinds[i] == kind:
                c = G.proof_read(self.proofs[192 * i:192 * i + 192])[2]
                out.append((i, B.ec_mul(B.FQ, c, G.batch_r(self.r16(i)))))
        return out

    def c_tree(self, kind):
        """the key's C-sum tree as k_tree_c forms it: node -> point (None: infinity), leaves npad + i, root 1"""
        t = {self.npad + i: None for i in range(self.npad)}
        for i, p in self.c_terms(kind):
            t[self.npad + i] = p
        for node in range(self.npad - 1, 0, -1):
            t[node] = B.ec_add(B.FQ, t[2 * node], t[2 * node + 1])
        return t

    def csum(self, kind):
        """batch_partial's csum[kind]: the running sum in slot order"""
        acc = None
        for _, p in self.c_terms(kind):
            acc = B.ec_add(B.FQ, acc, p)
        return acc

    def rotated(self, k):
        sl = lambda buf, w: buf[w * k:] + buf[:w * k]  # noqa: E731
        self._verify()
        return Case("%s@rot%d" % (self.name, k), sl(self.proofs, 192), sl(self.kinds, 1), sl(self.inputs, 288),
                    sl(self.r, 16), None if self.nin is None else sl(self.nin, 1),
                    self._st[k:] + self._st[:k], self._lhs[k:] + self._lhs[:k])


def _from_slots(name, slots, r):
    """slots: (kind, proof, rows, count | None)"""
    nin = None
    if any(s[3] is not None for s in slots):
        nin = bytes(G.KIND_NINPUTS[s[0]] if s[3] is None else s[3] for s in slots)
    return Case(name, b"".join(s[1] for s in slots), bytes(s[0] for s in slots), pack_rows([s[2] for s in slots]), r, nin)


# ------------------------------------------------------------------ sources
@functools.lru_cache(maxsize=None)
def sources():
    real = {e["name"]: e for e in load_golden("real_proofs.json")["proofs"]}
    return [real[s] for s in SRC_NAMES]


@functools.lru_cache(maxsize=None)
def pool():
    """POOL valid proofs: slot i is variant (i // 9) mod VARIANTS of source i mod 9, a variant being the
    oracle's re-randomisation (rerandomize_scalars of (RERAND_SEED, variant * 9 + source)); every slot is
    re-verified by the oracle (cpulib) and has its own seeded batch scalar row
    -> [(kind, proof, rows, None)], r rows"""
    srcs = sources()
    dec = [G.proof_read(bytes.fromhex(e["proof"])) for e in srcs]
    distinct = []
    for i in range(9 * VARIANTS):
        e = srcs[i % 9]
        t, s = G.rerandomize_scalars(RERAND_SEED, i)
        p = G.proof_bytes(G.rerandomize(dec[i % 9], pvks()[e["kind"]].vk.delta_g2, t, s))
        distinct.append((e["kind"], p, [bytes.fromhex(x) for x in e["inputs"]], None))
    out = [distinct[i % (9 * VARIANTS)] for i in range(POOL)]
    r = random.Random(RERAND_SEED).randbytes(16 * POOL)
    whole = _from_slots("pool", out, r)
    assert whole.statuses == [0] * POOL
    return out, [r[16 * i:16 * i + 16] for i in range(POOL)]


def _pool_case(name, idx):
    slots, rs = pool()
    return _from_slots(name, [slots[i] for i in idx], b"".join(rs[i] for i in idx))


# ------------------------------------------------------------------ 1. ragged sweep
@functools.lru_cache(maxsize=None)
def ragged_clean(n):
    """the first n pool slots: indices cycle over all nine sources"""
    return _pool_case("ragged%d" % n, range(n))


def corrupt_slots(case, slots, rot):
    """slot slots[q] gets class (rot + q) mod 6 of tests.test_gpu_configs.corrupt: the slot rides at
    position (rot + q) mod 6 of a six-proof batch that corrupt() corrupts at every position"""
    from tests.test_gpu_configs import corrupt
    assert len(slots) <= 6 and case.nin is None
    pos = [(rot + q) % 6 for q in range(len(slots))]
    src = {p: i for p, i in zip(pos, slots)}
    fill = [src.get(p, slots[0]) for p in range(6)]
    bp, bx, bad = corrupt(b"".join(case.proofs[192 * i:192 * i + 192] for i in fill), bytes(case.kinds[i] for i in fill),
                          b"".join(case.inputs[288 * i:288 * i + 288] for i in fill), 6, rot)
    assert bad == list(range(6))
    proofs, inputs = bytearray(case.proofs), bytearray(case.inputs)
    for p, i in src.items():
        proofs[192 * i:192 * i + 192] = bp[192 * p:192 * p + 192]
        inputs[288 * i:288 * i + 288] = bx[288 * p:288 * p + 288]
    return Case("%s+bad%s" % (case.name, list(slots)), proofs, case.kinds, inputs, case.r)


def bad_slots(n):
    return sorted({0, n // 2, n - 1})


@functools.lru_cache(maxsize=None)
def ragged_corrupt(n):
    """n >= 3: slot 0, one interior slot and slot n - 1 corrupted, the classes rotating with n"""
    assert n >= 3
    return corrupt_slots(ragged_clean(n), bad_slots(n), n)


def input0_plus1(slot):
    kind, proof, rows, cnt = slot
    x = (int.from_bytes(rows[0], "little") + 1).to_bytes(32, "little")
    return (kind, proof, [x] + list(rows[1:]), cnt)


@functools.lru_cache(maxsize=None)
def minimal_bad():
    """always-corrupted minimal batches: one input0_plus1 proof; one good and one bad proof, either order"""
    slots, rs = pool()
    bad = input0_plus1(slots[0])
    return [_from_slots("min1:bad", [bad], rs[0]),
            _from_slots("min2:good,bad", [slots[1], bad], rs[1] + rs[0]),
            _from_slots("min2:bad,good", [bad, slots[1]], rs[0] + rs[1])]


# ------------------------------------------------------------------ 2. kind mixes
MIXES = [(2,), (1,), (0,), (0, 1), (0, 2), (1, 2)]


@functools.lru_cache(maxsize=None)
def mix_clean(kinds, n):
    """n pool slots of the given kinds, the kinds taking turns (an absent key has an empty sum)"""
    slots, _ = pool()
    per = [[i for i in range(POOL) if slots[i][0] == k] for k in kinds]
    idx = [per[q % len(kinds)][q // len(kinds)] for q in range(n)]
    return _pool_case("mix%s:%d" % ("".join(map(str, kinds)), n), idx)


@functools.lru_cache(maxsize=None)
def mix_corrupt(kinds, n):
    return corrupt_slots(mix_clean(kinds, n), bad_slots(n), n + sum(kinds))


# ------------------------------------------------------------------ 3. all mutants in one batch
@functools.lru_cache(maxsize=None)
def mutant_items():
    """the 9 real proofs and the 71 builtin-key mutants, ordered so that the classes 0, 1, 2, 3, 4, 0
    sit in slots 0..5: the rotations MUTANT_ROTATIONS then put each class once in slot 0 and once in
    slot n - 1"""
    items = load_golden("real_proofs.json")["proofs"] + [
        m for m in load_golden("mutants.json")["mutants"] if m["vk"] == "builtin"]
    head = []
    for cls in (0, 1, 2, 3, 4, 0):
        head.append(next(e for e in items if e["status"] == cls and not any(e is h for h in head)))
    return head + [e for e in items if not any(e is h for h in head)]


MUTANT_ROTATIONS = [1, 2, 3, 4, 5]   # rotation k: slot 0 holds item k, slot n - 1 item k - 1


def _fixture_case(name, items, r, with_fixture=True):
    st = [e["status"] for e in items] if with_fixture else None
    lhs = [bytes.fromhex(e["lhs_gt"]) if e.get("lhs_gt") else None for e in items] if with_fixture else None
    return Case(name, b"".join(bytes.fromhex(e["proof"]) for e in items), bytes(e["kind"] for e in items),
                pack_rows([[bytes.fromhex(x) for x in e["inputs"]] for e in items]), r,
                bytes(len(e["inputs"]) for e in items), st, lhs)


@functools.lru_cache(maxsize=None)
def mutant_batch(with_fixture=True):
    """n = 80 (npad 128), each item's own n_inputs, seeded explicit r; with_fixture: statuses and LHS
    from the fixture, else from cpulib (the CPU tier compares the two)"""
    items = mutant_items()
    return _fixture_case("mutants", items, random.Random(80).randbytes(16 * len(items)), with_fixture)


# ------------------------------------------------------------------ 4. degenerate batches
def flip_c_sign(slot):
    """P -> P': the sign bit of the compressed C flipped (-C: a valid point, a failing proof)"""
    kind, proof, rows, cnt = slot
    p = bytearray(proof)
    p[144] ^= 0x20
    return (kind, bytes(p), rows, cnt)


DEGENERATE_KEYS = {0: (0, 1), 2: (5, 6)}   # key -> pool slots of P and Q (S1, S2; J1, J2)


@functools.lru_cache(maxsize=None)
def degenerate_sums(kind):
    """D1 - D4 for one key: name -> Case. P and P' (and Q, Q') share a scalar row, so r C and r (-C) meet"""
    slots, rs = pool()
    ip, iq = DEGENERATE_KEYS[kind]
    P, Q, rp, rq = slots[ip], slots[iq], rs[ip], rs[iq]
    assert P[0] == Q[0] == kind
    Pn, Qn = flip_c_sign(P), flip_c_sign(Q)
    sp = {"P": (P, rp), "P'": (Pn, rp), "Q": (Q, rq), "Q'": (Qn, rq)}
    shapes = {"D1": "P P", "D1x4": "P P P P", "D2": "P P'", "D2rev": "P' P", "D3a": "P P' Q", "D3b": "Q P P'",
              "D3c": "P Q P'", "D3right": "P P' Q Q'", "D4a": "P P P'", "D4b": "P P' P P'"}
    return {name: _from_slots("%s[k%d]" % (name, kind), [sp[t][0] for t in sh.split()],
                              b"".join(sp[t][1] for t in sh.split())) for name, sh in shapes.items()}


D_STATUSES = {"D1": [0, 0], "D1x4": [0] * 4, "D2": [0, 3], "D2rev": [3, 0], "D3a": [0, 3, 0], "D3b": [0, 0, 3],
              "D3c": [0, 0, 3], "D3right": [0, 3, 0, 3], "D4a": [0, 0, 3], "D4b": [0, 3, 0, 3]}


@functools.lru_cache(maxsize=None)
def nothing_live():
    """D5: the all-zero proof alone; three different decode failures (no compression flag on A, B at
    infinity, C outside the subgroup) -- statuses all 1, gt_out and partial the empty products"""
    mut = {m["name"]: m for m in load_golden("mutants.json")["mutants"] if m["vk"] == "builtin"}
    one = [mut["S1:zero_proof"]]
    three = [mut["S1:A_flag_cleared"], mut["O1:B_infinity"], mut["J1:C_not_in_subgroup"]]
    return [_fixture_case("D5:zero", one, bytes(range(16)), False),
            _fixture_case("D5:three", three, random.Random(5).randbytes(48), False)]


R_EXTREMES = [bytes(16), b"\xff" * 16, b"\xff" * 8 + bytes(8), bytes(8) + b"\xff" * 8,
              (1 << 63).to_bytes(8, "little") * 2]


@functools.lru_cache(maxsize=None)
def extreme_scalars():
    """D6: the nine sources (n = 9, npad 16) under a = b = 0, a = b = 2^64 - 1 (the top-window carry of
    msm_digit), (2^64 - 1, 0), (0, 2^64 - 1), (2^63, 2^63) and four seeded rows"""
    slots, _ = pool()
    r = b"".join(R_EXTREMES) + random.Random(6).randbytes(16 * 4)
    return _from_slots("D6", slots[:9], r)


@functools.lru_cache(maxsize=None)
def extreme_inputs():
    """D7: slots with all inputs zero, all inputs r - 1, one input = r, one input = 2^256 - 1, n_inputs
    one short, n_inputs one long -- first, last and interior among valid proofs"""
    slots, rs = pool()
    le = lambda v: v.to_bytes(32, "little")  # noqa: E731

    def with_rows(slot, f, cnt=None):
        return (slot[0], slot[1], f(list(slot[2])), cnt)

    def one(rows, j, v):
        rows[j] = le(v)
        return rows
    n_of = lambda s: len(s[2])  # noqa: E731
    special = [
        with_rows(slots[0], lambda rows: [le(0)] * len(rows)),               # spend, all zero
        slots[10],
        with_rows(slots[5], lambda rows: [le(B.R - 1)] * len(rows)),          # sprout, all r - 1
        slots[11],
        with_rows(slots[2], lambda rows: one(rows, 2, B.R)),                  # output, input 2 = r
        with_rows(slots[6], lambda rows: one(rows, 8, (1 << 256) - 1)),       # sprout, last input 2^256 - 1
        slots[12],
        with_rows(slots[1], lambda rows: rows, n_of(slots[1]) - 1),           # spend, one short
        with_rows(slots[7], lambda rows: rows, n_of(slots[7]) - 1),           # sprout, one short
        slots[13], slots[14],
        with_rows(slots[3], lambda rows: rows, n_of(slots[3]) + 1),           # output, one long
        slots[15],
        with_rows(slots[9], lambda rows: rows, n_of(slots[9]) + 1),           # spend, one long
    ]
    return _from_slots("D7", special, random.Random(7).randbytes(16 * len(special)))


D7_STATUSES = [3, 0, 3, 0, 4, 4, 0, 2, 2, 0, 0, 2, 0, 2]


def degenerate_cases():
    out = []
    for kind in DEGENERATE_KEYS:
        out += list(degenerate_sums(kind).values())
    return out + nothing_live() + [extreme_scalars(), extreme_inputs()]


# ------------------------------------------------------------------ 5. API corners
@functools.lru_cache(maxsize=None)
def empty_batch():
    return Case("empty", b"", b"", b"", b"")


def all_mix_cases():
    return [f(k, n) for k, n in itertools.product(MIXES, MIX_SIZES) for f in (mix_clean, mix_corrupt)]
