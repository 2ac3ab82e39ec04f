"""Case builders for the PGHR13 batch-check edge tests (tests/test_pghr13_edges.py on the CPU,
tests/test_gpu_pghr13_edges.py on the GPU): ragged sizes under every launch shape of
zg_pghr13_verify's batch path (zebra_amd/csrc/zg_pghr13.hip: k_pghr_straus<B>, k_pghr_bseg with K
proofs per lane, the per-call chunk loop of zg_calls.hip), one failing proof per call in the slots where a
lane map ends, slots the batch excludes, calls with nothing live.

Every expectation here comes from the oracle alone: a slot's status is that of the C++ restatement of
the reference's check (tests/cpulib.pg_verify), cross-checked against the fixture's own `status`; the
one status the reference cannot express -- an input >= r is not constructible as bn::Fr, include/zg.h
ZG_STATUS_INPUT_NONCANONICAL -- is restated here as that rule. The lane maps are restated from the
kernels' comments. Nothing here touches the GPU."""
import functools

from oracle import bn254 as B
from tests import cpulib
from tests.conftest import load_golden

OK, DECODE_INVALID, VERIFY_FAILED, INPUT_NONCANONICAL = 0, 1, 3, 4   # include/zg.h ZG_STATUS_*

# each breaks exactly one of the five equalities of oracle/pghr13.py verify, in their order there
MUTANTS = ["mut_a_prime_x_moved", "mut_b_prime_x_moved", "mut_c_prime_x_moved", "mut_k_x_moved", "mut_h_sign"]
DECODE_BAD = "mut_b_not_in_subgroup"    # decided on the side stream (b's decode + subgroup check)
NONCANON = "noncanon"                   # valid case 0 with input 2 = r

# (B, K) as the environment a context is created under; {}: by size (B = 1, K = 1 at every size used here)
SHAPES = [{}, {"ZG_STRAUS_B": 2, "ZG_BSEG_K": 2}, {"ZG_STRAUS_B": 1, "ZG_BSEG_K": 8},
          {"ZG_STRAUS_B": 4, "ZG_BSEG_K": 4}, {"ZG_STRAUS_B": 2, "ZG_BSEG_K": 8}, {"ZG_STRAUS_B": 4, "ZG_BSEG_K": 1},
          {"ZG_STRAUS_B": 4, "ZG_BSEG_K": 3}, {"ZG_STRAUS_B": 1, "ZG_BSEG_K": 64}]
UNSEEDED_SHAPE = {"ZG_STRAUS_B": 4, "ZG_BSEG_K": 8}
# 521: three Straus blocks with a tail at B = 4 (G = 131), two segment blocks at K = 8 (G = 66), more than
# one k_pghr_ssum chunk for S1 (its 4 families x G partials: 2,084 at B = 1, 1,044 at B = 2)
SWEEP_SIZES = [1, 2, 5, 65, 130, 521]
# G = ceil(n / B) > 1,024 for B = 2 / 4: one family's partials cross a ZG_PGHR_SSUM_CH chunk
LARGE_SIZES = [2063, 4099]
VALID_ORDER = [521, 5, 130, 1, 4099, 2, 65, 2063]   # a smaller call reuses the arena after a larger one
CHUNK_SIZES = [64, 65, 129, 200]
CHUNK_ENVS = [{"ZG_PGHR_CHUNK": 64}, {"ZG_PGHR_CHUNK": 1}]   # 1 clamps to 64
DEFAULT_CHUNK = 65536
MAX_POSITIONS = 8


def shape_id(env):
    return ",".join("%s=%s" % kv for kv in env.items()) or "default"


# ------------------------------------------------------------------ the launch shape, restated
def auto_shape(n):
    """bn_pghr13_shape (zg_pghr13.hip) for one chunk of n proofs with nothing forced"""
    k = 1
    while k < 8 and n // (2 * k) >= 8192:
        k *= 2
    return {"straus_b": 2 if n >= 28672 else 1, "bseg_k": k, "halves": 2 if n < 32768 else 1,
            "p7_side": 1 if n >= 32768 else 0}


# one below and at every threshold of auto_shape: K = 1, 2, 4, 8 from 0, 16,384, 32,768, 65,536; B = 2 from
# 28,672; halves and p7_side at 32,768
THRESHOLD_SIZES = [0, 1, 16383, 16384, 28671, 28672, 32767, 32768, 65535, 65536]


def expected_shape(env, n, chunk=DEFAULT_CHUNK):
    """zg_pghr13_shape's answer on a context created under env: zg_create's clamps (B outside {1, 2, 4} and
    K <= 0 mean by size, K > 32 is 32, the chunk within [64, 65,536]) over auto_shape of the first chunk"""
    chunk = max(64, min(DEFAULT_CHUNK, env.get("ZG_PGHR_CHUNK", chunk)))
    out = dict(auto_shape(min(n, chunk)), chunk=chunk)
    if env.get("ZG_STRAUS_B") in (1, 2, 4):
        out["straus_b"] = env["ZG_STRAUS_B"]
    if env.get("ZG_BSEG_K", 0) > 0:
        out["bseg_k"] = min(32, env["ZG_BSEG_K"])
    return out


# ------------------------------------------------------------------ lane maps, restated
def _strided(n, per):
    """lane g carries the proofs g + k G, k < per, G = ceil(n / per), those below n (k_pghr_straus:
    "lane (family f, group g) carries the B proofs g, g + G, .."; k_pghr_bseg: "group g = 64 b + l carries
    the proofs g, g + G, .., g + (K - 1) G") -> per lane the list of its proofs"""
    g_count = (n + per - 1) // per
    return [[g + k * g_count for k in range(per) if g + k * g_count < n] for g in range(g_count)]


def straus_slots(n, b):
    return _strided(n, b)


def bseg_slots(n, k):
    return _strided(n, k)


def critical_positions(n, b, k, cap=MAX_POSITIONS):
    """the slots where a lane map of the call ends or wraps: {0, n-1, G_B-1, G_B, (B-1) G_B, G_K-1, G_K,
    (K-1) G_K, 63, 64} within [0, n), without repeats, at most cap of them. Order: n-1, 0 and the first
    slot of each map's last stride come first (a cap never drops them), then the stride edges, then the
    wave edge; a position's index q in this list picks its mutant class, (n + q) mod 5."""
    gb, gk = (n + b - 1) // b, (n + k - 1) // k
    order = [n - 1, 0, (b - 1) * gb, (k - 1) * gk, gb - 1, gb, gk - 1, gk, 63, 64]
    out = []
    for p in order:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out[:cap]


def mutant_class(n, q):
    return (n + q) % len(MUTANTS)


def chunk_positions(n, chunk=64):
    """slot 63, slot 64, slot n-1 and the first slot of the last chunk, those within [0, n)"""
    out = []
    for p in (63, 64, n - 1, (n - 1) // chunk * chunk):
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


# ------------------------------------------------------------------ slots and the oracle
@functools.lru_cache(maxsize=None)
def slots():
    """name -> (proof, [inputs], the fixture's status or None): the nine valid cases of
    tests/golden/pghr13.json as "valid0".."valid8", the mutants under their fixture names, NONCANON"""
    by = {c["name"]: c for c in load_golden("pghr13.json")["cases"]}
    valid = [c for c in load_golden("pghr13.json")["cases"] if c["status"] == OK][:9]
    assert len(valid) == 9
    conv = lambda c: (bytes.fromhex(c["proof"]), tuple(bytes.fromhex(x) for x in c["inputs"]), c["status"])  # noqa: E731
    out = {"valid%d" % i: conv(c) for i, c in enumerate(valid)}
    for name in MUTANTS + [DECODE_BAD]:
        out[name] = conv(by[name])
    p, ins, _ = out["valid0"]
    out[NONCANON] = (p, ins[:2] + (B.R.to_bytes(32, "little"),) + ins[3:], None)
    return out


@functools.lru_cache(maxsize=None)
def oracle_statuses():
    """name -> status: tests/cpulib.pg_verify over every slot whose inputs are all below r (one call), equal
    to the fixture's status where the slot is a fixture case; INPUT_NONCANONICAL for a row with an input
    >= r (the reference cannot form such an Fr; the C++ restatement would reduce it)"""
    sl = slots()
    canon = [k for k, (_, ins, _) in sl.items() if all(int.from_bytes(x, "little") < B.R for x in ins)]
    got = cpulib.pg_verify(cpulib.load_pghr13(), [sl[k][0] for k in canon], [list(sl[k][1]) for k in canon], threads=8)
    out = dict(zip(canon, got))
    for k in sl:
        out.setdefault(k, INPUT_NONCANONICAL)
    return out


class Case:
    """one call: per slot the name of what it holds -> the ABI's packed buffers and the oracle's statuses"""

    def __init__(self, name, names):
        self.name, self.names, self.n = name, list(names), len(names)

    @property
    def proofs(self):
        sl = slots()
        return b"".join(sl[k][0] for k in self.names)

    @property
    def inputs(self):
        sl = slots()
        return b"".join(b"".join(sl[k][1]) + bytes(32 * (9 - len(sl[k][1]))) for k in self.names)

    @property
    def counts(self):
        sl = slots()
        return bytes(len(sl[k][1]) for k in self.names)

    @property
    def statuses(self):
        st = oracle_statuses()
        return [st[k] for k in self.names]

    @property
    def fixture_statuses(self):
        """the fixture's own status per slot (None where the slot is no fixture case)"""
        sl = slots()
        return [sl[k][2] for k in self.names]

    @property
    def fails(self):
        """the call's batch check must fail: some slot takes part in it and is false"""
        return VERIFY_FAILED in self.statuses


def _filler(n):
    return ["valid%d" % (i % 9) for i in range(n)]


def all_valid(n):
    return Case("valid%d" % n, _filler(n))


def one_bad(n, pos, cls):
    """n valid proofs but slot pos, which holds the mutant that breaks equality cls + 1 alone"""
    names = _filler(n)
    names[pos] = MUTANTS[cls]
    return Case("n%d@%d:%s" % (n, pos, MUTANTS[cls]), names)


def position_sweep(n, b, k, cap=MAX_POSITIONS):
    """one call per critical position of (n, B, K), its mutant class rotating as (n + q) mod 5"""
    return [one_bad(n, p, mutant_class(n, q)) for q, p in enumerate(critical_positions(n, b, k, cap))]


def large_bad(n):
    """a large size with one mutant in its last slot (position index 0 of critical_positions)"""
    return one_bad(n, n - 1, mutant_class(n, 0))


def excluded(n):
    """the decode-invalid case and the non-canonical row at slots 0 and n-1 among valid proofs, both ways
    round (n = 1: each alone): the batch leaves them out and still passes"""
    out = []
    for first, last in ((DECODE_BAD, NONCANON), (NONCANON, DECODE_BAD)):
        names = _filler(n)
        names[n - 1] = last
        names[0] = first
        out.append(Case("n%d:%s..%s" % (n, names[0], names[n - 1]), names))
    return out


def nothing_live():
    """calls in which no proof reaches the batch check: every sum is infinity and no b pair exists"""
    return [Case("dead1", [DECODE_BAD]), Case("dead3", [DECODE_BAD, NONCANON, DECODE_BAD]),
            Case("dead65", [DECODE_BAD] * 65)]
