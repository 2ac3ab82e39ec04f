"""Block-level Groth16 collector -- the caller side of the boundary.

Restates how the reference's chain acceptor reaches the proof checks, so that a whole block
(or import window) is verified with ONE batch call while the reported error stays exactly the
reference's:

  ChainAcceptor::check_transactions   verification/src/accept_chain.rs:76-81
      rayon fold/reduce over transactions: the LOWEST failing tx index wins
  TransactionAcceptor::check          verification/src/accept_transaction.rs:68-84
      ... -> eval (sighash) -> join_split.check -> sapling.check
  JoinSplitVerification::check        accept_transaction.rs:649-657
      ed25519 JoinSplit signature -> JoinSplitProof::check -> JoinSplit nullifiers
  JoinSplitProof::check               accept_transaction.rs:575-596
      per description i: sprout::verify (-> InvalidJoinSplit(i)), then tree_cache.continue_root
  SaplingVerification                 accept_transaction.rs:700-714 (SaplingProof::check)
      accept_sapling (sapling.rs:75-98): per spend (cv, anchor, rk, spend_auth_sig, proof),
      per output (cv, cmu, epk, proof), binding signature -> any failure is InvalidSapling;
      then Sapling nullifiers

The checks that are not proofs or signatures (tree roots, nullifiers, the transparent checks
before the shielded stages) are evaluated by the caller exactly as today and handed in as
outcomes; the Ed25519 JoinSplit signature too, unless the transaction carries it (Tx.js_sig):
then every such signature of the window is verified in ONE zg_ed25519_verify call (SURVEY.md 8(f)
f5; accept_transaction.rs:649-653 -> crypto::verify_ed25519 crypto/src/lib.rs:298-305). The script
interpreter of the transparent inputs stays with the caller too, but the secp256k1 signature checks
under it can be handed in (Tx.ecdsa_checks): the caller runs TransactionEval::check
(accept_transaction.rs:363-422) once with a recording checker that answers true, every recorded check
of the window is verified in ONE zg_ecdsa_verify call, and only a transaction with a failed check has
its script run repeated with the real verdicts (Tx.eval_rerun). The signature hashes themselves can be left to
the GPU as well: a transaction that carries its serialized bytes (Tx.raw, Tx.branch_id) and
no sighash gets the no-input hash the acceptor computes (accept_transaction.rs:374-386), and its checks may be
handed in without their hash (Tx.ecdsa_requests: script code, hashtype and amount instead); all of the window's
are computed in ONE zg_sighash call before the signature batches. A transaction whose inputs are all pay-to-pubkey-hash
or pay-to-pubkey spends (zg.script_class says so before any interpreter runs) needs no script run at all (SURVEY.md
8(f) f15): it carries the outputs it spends (Tx.prevouts) instead of checks, and every such input of the window is
verified -- HASH160, the encoding check, the signature hash and the signature -- in ONE zg_inputs_verify call. A
window whose script_flags carry zg.SCRIPT_TEMPLATE_MULTISIG opts in to m-of-n OP_CHECKMULTISIG inputs as well, bare or
behind pay-to-script-hash (zg.script_match names the class): the flags go to the call as they
are. A transaction marked Tx.shielded carries no sliced fields at all: its whole JoinSplit and
Sapling stage -- the hash, the Ed25519 signature, the JoinSplit and Sapling proofs with their preparation, the
RedJubjub signatures -- is read from Tx.raw in ONE zg_shielded_verify call for the window, and the caller's tree and
nullifier outcomes (Tx.tree_errors, js_nullifier_error, sapling_nullifier_error) are placed around its verdict. That
call also checks the default binding signature of a v4 transaction without spends and outputs, as the reference does;
the six-call path below does not. For every other transaction the
collector prepares every public input of
the window in one zg_prep_batch call (the Sapling descriptions' Jubjub decodes on the GPU, the
JoinSplits on host threads; without a context, the per-description zg_prep_* host functions),
verifies all Groth16 proofs of the window in
one zg_verify_batch call and all PGHR13 proofs of pre-Sapling JoinSplits (sprout.rs:61-67,
inputs Input::into_bn_frs via zg_prep_joinsplit_bn) in one zg_pghr13_verify call, and
re-injects the per-proof statuses in reference order: a PHGR description that fails to decode
(InvalidEncoding) or to verify (InvalidPGHRProof) is InvalidJoinSplit(index), at its place among
the transaction's descriptions, before its tree_cache.continue_root (accept_transaction.rs:575-592).
"""
from dataclasses import dataclass, field
from typing import Callable, List, Optional

from . import zg

OK = zg.STATUS_OK


@dataclass
class JoinSplit:
    """one JoinSplit description (chain/src/join_split.rs:169-186)"""
    anchor: bytes
    random_seed: bytes
    nullifiers: List[bytes]
    macs: List[bytes]
    commitments: List[bytes]
    vpub_old: int
    vpub_new: int
    zkproof: bytes                    # 192 B Groth16 (v4+) or 296 B PGHR13
    groth: bool = True
    pghr_ok: Optional[bool] = None    # a PGHR13 verdict the caller already holds (None: the GPU
                                      # verifies the description in the window's PGHR13 call)
    tree_error: Optional[str] = None  # caller's tree_cache.continue_root outcome (None = ok)


@dataclass
class Spend:
    cv: bytes
    anchor: bytes
    nullifier: bytes
    rk: bytes
    zkproof: bytes
    sig_ok: bool = True               # caller's spend_auth_sig (RedJubjub) verdict, used when
    spend_auth_sig: Optional[bytes] = None   # ... this is None; else verified on the GPU


@dataclass
class Output:
    cv: bytes
    cmu: bytes
    epk: bytes
    zkproof: bytes


@dataclass
class EcdsaCheck:
    """one signature check a script run asked its checker for (TransactionSignatureChecker::
    verify_signature, script/src/verify.rs:60-67): the key and the DER signature without its hashtype
    byte as the script pushed them, and the 32-byte sighash of that input"""
    input_index: int
    pubkey: bytes
    sig: bytes
    sighash: bytes


@dataclass
class EcdsaRequest:
    """an EcdsaCheck whose sighash is still to be computed: the arguments the checker would pass to
    TransactionInputSigner::signature_hash (script/src/verify.rs:60-67, sign.rs:152-160) -- the script code after
    OP_CODESEPARATOR / signature removal, the hashtype byte the signature carried (as u32) and the amount of
    the output the input spends. Needs Tx.raw"""
    input_index: int
    pubkey: bytes
    sig: bytes
    script_code: bytes
    hashtype: int
    amount: int


@dataclass
class Prevout:
    """the output an input spends: its script and its value (the `previous_output` the acceptor looks up,
    accept_transaction.rs:363-422)"""
    script_pubkey: bytes
    amount: int


@dataclass
class Tx:
    """the shielded-proof view of one transaction, with the caller's non-Groth16 outcomes"""
    pre_error: Optional[str] = None           # first failing check before the JoinSplit stage
    js_pubkey: Optional[bytes] = None
    js_sig_ok: bool = True                    # caller's Ed25519 verdict, used when js_sig is None
    joinsplits: List[JoinSplit] = field(default_factory=list)
    js_nullifier_error: Optional[str] = None
    spends: List[Spend] = field(default_factory=list)
    outputs: List[Output] = field(default_factory=list)
    binding_ok: bool = True                   # caller's binding_sig verdict, used when binding_sig is None
    sapling_nullifier_error: Optional[str] = None
    # the Sapling signature checks on the GPU: the no-input ZIP-243 sighash the
    # acceptor computes (accept_transaction.rs:374-386), valueBalance and the binding signature
    sighash: Optional[bytes] = None
    value_balance: int = 0
    binding_sig: Optional[bytes] = None
    # the JoinSplit signature on the GPU: the 64-byte Ed25519 signature over the
    # same sighash, checked against js_pubkey (accept_transaction.rs:649-653)
    js_sig: Optional[bytes] = None
    # the transparent inputs' ECDSA checks on the GPU. A script's run depends on its
    # checker only through the booleans it returns, so the caller runs TransactionEval::check once with a
    # recording checker that answers true and notes every check here; if the GPU confirms them all, that
    # run was the reference's run (and pre_error, which then covers only the checks before eval, stands).
    # Otherwise eval_rerun(lookup) repeats the run with lookup(pubkey, sig, sighash) -> bool as the
    # checker and returns the reference's eval error, or None
    ecdsa_checks: List[EcdsaCheck] = field(default_factory=list)
    eval_rerun: Optional[Callable] = None
    # the signature hashes on the GPU: the serialized transaction and its consensus
    # branch id. With raw set and sighash None, the no-input sighash (hashtype 1) is computed in the window's
    # zg_sighash call; ecdsa_requests are resolved to ecdsa_checks by the same call. eval_rerun of a transaction
    # with requests may ask lookup(input_index, pubkey, sig, script_code, hashtype) -> bool: no sighash needed
    raw: Optional[bytes] = None
    branch_id: Optional[int] = None
    ecdsa_requests: List[EcdsaRequest] = field(default_factory=list)
    # the whole script check of template inputs on the GPU: one Prevout per input, set only when
    # zg.script_class names every input of the transaction a template (P2PKH or P2PK; with SCRIPT_TEMPLATE_MULTISIG in
    # the window's script_flags, zg.script_match and the two multisig classes as well). Needs raw and branch_id;
    # ecdsa_checks, ecdsa_requests and eval_rerun must then be empty: no interpreter runs for this transaction
    prevouts: Optional[List[Prevout]] = None
    # the whole JoinSplit and Sapling stage from the serialized bytes on the GPU, opt-in: with
    # shielded set the transaction carries raw and branch_id, and js_pubkey, js_sig, joinsplits, spends, outputs,
    # sighash and binding_sig stay empty -- nothing is sliced out on the host. The caller's tree_cache.continue_root
    # outcomes go in tree_errors (one entry per JoinSplit description, None = ok; may be shorter than the list)
    shielded: bool = False
    tree_errors: List[Optional[str]] = field(default_factory=list)


_POOL = None
_PAR_MIN = 32   # prep jobs below this run inline (a pool round trip costs more than they do)
# windows from this many descriptions go through zg_prep_batch (the GPU); below, the host functions:
# a lone 9-description block took 6.6 ms with host prep and 8.6 ms with the batched call (its copies
# and launch), a 401-description block 12.1 -> 9.8 ms, a 9,609-description window 383 -> 35 ms
# (tools/bench_config5.py; profiles/r06q_config5.txt)
_GPU_PREP_MIN = 64


def _prep_pool():
    """host threads for the public-input preparation (Jubjub point decodes, small-order checks,
    multipacking: ~0.35 ms of C per Sapling description); the prep functions are ctypes calls into
    libzg.so, which release the GIL, so a window's descriptions decode in parallel like the
    reference's rayon fan-out over transactions (accept_chain.rs:76-81). Sized like the bench's
    CPU share: OMP_NUM_THREADS when set, else every usable CPU (at most 64)."""
    global _POOL
    if _POOL is None:
        import concurrent.futures
        import os
        try:
            n = len(os.sched_getaffinity(0))
        except AttributeError:
            n = os.cpu_count() or 1
        omp = os.environ.get("OMP_NUM_THREADS", "")
        if omp.isdigit() and int(omp) > 0:
            n = min(n, int(omp))
        _POOL = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(64, n)))
    return _POOL


def _run_prep(job):
    fn, args = job
    try:
        return fn(*args)
    except zg.PrepError as e:
        return e


def _jobs(txs):
    """the window's preparation jobs in reference order: (PREP_KIND_*, arguments of the prep function)"""
    jobs = []
    for tx in txs:
        for d in tx.joinsplits:
            if tx.js_pubkey is None or (not d.groth and d.pghr_ok is not None):
                continue
            jobs.append((zg.PREP_KIND_JOINSPLIT if d.groth else zg.PREP_KIND_JOINSPLIT_BN,
                         (d.anchor, d.random_seed, d.nullifiers, d.macs, d.commitments, d.vpub_old, d.vpub_new,
                          tx.js_pubkey)))
        for s in tx.spends:
            jobs.append((zg.PREP_KIND_SPEND, (s.cv, s.anchor, s.nullifier, s.rk)))
        for o in tx.outputs:
            jobs.append((zg.PREP_KIND_OUTPUT, (o.cv, o.cmu, o.epk)))
    return jobs


_PREP_FN = {zg.PREP_KIND_SPEND: zg.prep_spend, zg.PREP_KIND_OUTPUT: zg.prep_output,
            zg.PREP_KIND_JOINSPLIT: zg.prep_joinsplit, zg.PREP_KIND_JOINSPLIT_BN: zg.prep_joinsplit_bn}


_PAD = {zg.PREP_KIND_SPEND: bytes(zg.PREP_FIELD_BYTES - 128), zg.PREP_KIND_OUTPUT: bytes(zg.PREP_FIELD_BYTES - 96)}


def _fields(jobs):
    """the window's zg_prep_batch field rows: the Sapling descriptions' 32-byte fields joined as they are
    (one join for the window), the JoinSplits through zg.prep_fields; a field of the wrong size is
    reported by zg.prep_fields"""
    out = []
    for k, a in jobs:
        if k == zg.PREP_KIND_SPEND or k == zg.PREP_KIND_OUTPUT:
            out.extend(a)
            out.append(_PAD[k])
        else:
            out.append(zg.prep_fields(k, *a))
    f = b"".join(out)
    if len(f) != zg.PREP_FIELD_BYTES * len(jobs):
        f = b"".join(zg.prep_fields(k, *a) for k, a in jobs)   # raises on the malformed description
    return f


def _prepare(jobs, ctx):
    """-> per job: the packed 288-byte input row, or a PrepError. With a context: ONE zg_prep_batch call
    for the window (Sapling descriptions on the GPU, JoinSplits on host threads); without: the
    per-description host functions (in parallel for a large window)."""
    if ctx is not None and len(jobs) >= _GPU_PREP_MIN:
        kinds = bytes(k for k, _ in jobs)
        fields = _fields(jobs)
        rows, codes = ctx.prep_batch(kinds, fields)
        return [zg.PrepError(c) if c else rows[zg.INPUT_STRIDE * i:zg.INPUT_STRIDE * (i + 1)]
                for i, c in enumerate(codes)]
    calls = [(_PREP_FN[k], a) for k, a in jobs]
    if len(calls) >= _PAR_MIN:
        done = list(_prep_pool().map(_run_prep, calls, chunksize=16))
    else:
        done = [_run_prep(c) for c in calls]
    return [d if isinstance(d, zg.PrepError) else zg.pack_inputs([d]) for d in done]


def _queue(txs, ctx=None):
    """prepare inputs; returns (Groth16 items (kind, proof, 288-byte input row, n inputs), PGHR13 items
    (proof, inputs), per-tx plans). A plan entry refers to a queued proof by index ("proof" / "pghr"),
    or carries a prep error or a caller verdict. The window's preparation runs first (_prepare), then
    the items and plans are assembled in reference order."""
    res = iter(_prepare(_jobs(txs), ctx))
    items, pghr, plans = [], [], []
    for tx in txs:
        js_plan, sp_plan, out_plan = [], [], []
        for d in tx.joinsplits:
            if tx.js_pubkey is None or (not d.groth and d.pghr_ok is not None):
                js_plan.append(("caller", bool(d.pghr_ok)))
                continue
            row = next(res)
            if isinstance(row, zg.PrepError):   # (the JoinSplit preps raise no PrepError)
                raise row
            if not d.groth:
                js_plan.append(("pghr", len(pghr)))
                pghr.append((bytes(d.zkproof), [row[32 * j:32 * j + 32] for j in range(9)]))
                continue
            js_plan.append(("proof", len(items)))
            items.append((zg.KIND_SPROUT, bytes(d.zkproof), row, 9))
        for s in tx.spends:
            row = next(res)
            if isinstance(row, zg.PrepError):
                sp_plan.append(("prep", row.name))
                continue
            sp_plan.append(("proof", len(items)))
            items.append((zg.KIND_SPEND, bytes(s.zkproof), row, 7))
        for o in tx.outputs:
            row = next(res)
            if isinstance(row, zg.PrepError):
                out_plan.append(("prep", row.name))
                continue
            out_plan.append(("proof", len(items)))
            items.append((zg.KIND_OUTPUT, bytes(o.zkproof), row, 5))
        plans.append((js_plan, sp_plan, out_plan))
    return items, pghr, plans


def _sig_verdicts(txs, ctx, verify_sigs, sapling_bvk):
    """spend_auth_sig and binding_sig verdicts of the transactions that carry a sighash (the rest
    keep the caller's booleans): the binding verification keys in one zg_sapling_bvk call, every
    signature of the window in ONE zg_redjubjub_verify call (accept_spend sapling.rs:119-137,
    accept_sapling_final :216-244). Returns (per-tx spend sig oks, per-tx binding ok)."""
    if verify_sigs is None:
        verify_sigs = ctx.redjubjub_verify if ctx is not None else None
    if sapling_bvk is None:
        sapling_bvk = ctx.sapling_bvk if ctx is not None else None
    sp_ok = [[s.sig_ok for s in tx.spends] for tx in txs]
    bind_ok = [tx.binding_ok for tx in txs]
    need = [i for i, tx in enumerate(txs) if tx.sighash is not None and (tx.spends or tx.outputs)]
    if not need:
        return sp_ok, bind_ok
    if verify_sigs is None or sapling_bvk is None:
        raise zg.ZgError(-1, "transactions carry a sighash but no signature backend was given "
                             "(pass ctx=, or verify_sigs= and sapling_bvk=)")
    bvks = sapling_bvk([([s.cv for s in txs[i].spends], [o.cv for o in txs[i].outputs], txs[i].value_balance)
                        for i in need])
    items, where = [], []
    for i, (st, bvk) in zip(need, bvks):
        tx = txs[i]
        for j, s in enumerate(tx.spends):
            if s.spend_auth_sig is not None:
                items.append((s.rk, s.spend_auth_sig, bytes(s.rk) + bytes(tx.sighash), zg.GEN_SPEND_AUTH))
                where.append((i, j))
        if tx.binding_sig is not None:
            if st == 0:
                items.append((bvk, tx.binding_sig, bvk + bytes(tx.sighash), zg.GEN_BINDING))
                where.append((i, None))
            else:   # a cv that does not decode fails its own description first; i64::MIN: InvalidBalanceValue
                bind_ok[i] = False
    if items:
        oks = verify_sigs(*[list(x) for x in zip(*items)])
        for (i, j), ok in zip(where, oks):
            if j is None:
                bind_ok[i] = ok
            else:
                sp_ok[i][j] = ok
    return sp_ok, bind_ok


def _js_sig_verdicts(txs, ctx, verify_js_sigs):
    """the Ed25519 JoinSplit signature verdict of each transaction: the caller's js_sig_ok, or, for a
    transaction with JoinSplits that carries js_sig and js_pubkey, the status of the window's ONE
    zg_ed25519_verify call (any non-zero status is the reference's JoinSplitSignature error:
    crypto::verify_ed25519 maps every dalek error to Err, accept_transaction.rs:649-653)."""
    ok = [tx.js_sig_ok for tx in txs]
    need = [i for i, tx in enumerate(txs)
            if tx.js_sig is not None and tx.joinsplits and tx.js_pubkey is not None]
    if not need:
        return ok
    if any(txs[i].sighash is None for i in need):
        raise zg.ZgError(-1, "a transaction carries js_sig but no sighash")
    if verify_js_sigs is None:
        if ctx is None:
            raise zg.ZgError(-1, "transactions carry a JoinSplit signature but no Ed25519 backend was given "
                                 "(pass ctx= or verify_js_sigs=)")
        verify_js_sigs = ctx.ed25519_verify
    sts = verify_js_sigs([bytes(txs[i].js_pubkey) for i in need], [bytes(txs[i].js_sig) for i in need],
                         [bytes(txs[i].sighash) for i in need])
    for i, st in zip(need, sts):
        ok[i] = st == zg.ED_OK
    return ok


def _resolve_sighashes(txs, ctx, sighash):
    """-> (txs with every sighash in place, resolve). The transactions that carry raw bytes and lack their
    no-input sighash or carry ecdsa_requests are copied with sighash set and the requests appended to
    ecdsa_checks as EcdsaChecks, all from ONE sighash(raws, branch_ids, items) call (default ctx.sighash);
    the others are passed through untouched. resolve(i, input_index, script_code, hashtype) -> the sighash of
    a request of transaction i (computed by a further call if the window's did not hold it). A transaction
    or item the GPU does not hash (a status other than SIGHASH_OK) raises: the caller hashes it."""
    need = [i for i, tx in enumerate(txs)
            if tx.raw is not None and ((tx.sighash is None and not tx.shielded) or tx.ecdsa_requests)]
    bad = [i for i, tx in enumerate(txs) if tx.raw is None and tx.ecdsa_requests]
    if bad:
        raise zg.ZgError(-1, "transaction %d carries ecdsa_requests but no raw bytes" % bad[0])
    if not need:
        return txs, None
    if sighash is None:
        if ctx is None:
            raise zg.ZgError(-1, "transactions carry raw bytes but no sighash backend was given (pass ctx= or sighash=)")
        sighash = ctx.sighash
    from dataclasses import replace

    def run(pairs):
        """pairs: (window index, (input index | None, script code, amount, hashtype)) -> hashes"""
        idx = sorted({i for i, _ in pairs})
        pos = {i: k for k, i in enumerate(idx)}
        _, hashes, status = sighash([bytes(txs[i].raw) for i in idx], [txs[i].branch_id or 0 for i in idx],
                                    [(pos[i],) + tuple(it) for i, it in pairs])
        for (i, it), st in zip(pairs, status):
            if st != zg.SIGHASH_OK:
                raise zg.ZgError(-1, "transaction %d: the signature hash of input %r was not computed (ZG_SIGHASH "
                                     "status %d); hash this transaction on the host" % (i, it[0], st))
        return hashes

    pairs = []
    for i in need:
        if txs[i].sighash is None and not txs[i].shielded:
            pairs.append((i, (None, b"", 0, 1)))
        pairs += [(i, (r.input_index, bytes(r.script_code), r.amount, r.hashtype)) for r in txs[i].ecdsa_requests]
    known = {(i, it[0], it[1], it[3]): h for (i, it), h in zip(pairs, run(pairs))}
    out = list(txs)
    for i in need:
        tx = txs[i]
        checks = list(tx.ecdsa_checks) + [
            EcdsaCheck(r.input_index, r.pubkey, r.sig, known[(i, r.input_index, bytes(r.script_code), r.hashtype)])
            for r in tx.ecdsa_requests]
        out[i] = replace(tx, sighash=tx.sighash if tx.sighash is not None else known.get((i, None, b"", 1)),
                         ecdsa_checks=checks)

    def resolve(i, input_index, script_code, hashtype):
        key = (i, input_index, bytes(script_code), hashtype)
        if key not in known:
            amounts = {r.amount for r in txs[i].ecdsa_requests if r.input_index == input_index}
            if len(amounts) != 1:
                raise zg.ZgError(-1, "transaction %d: no single amount is known for input %d" % (i, input_index))
            known[key] = run([(i, (input_index, key[2], amounts.pop(), hashtype))])[0]
        return known[key]
    return out, resolve


def _eval_errors(txs, ctx, verify_ecdsa, resolve=None):
    """-> eval_error(tx): the reference's TransactionEval error of a transaction (None: the scripts pass).
    Every recorded check of the window goes through ONE verify_ecdsa call; a transaction whose checks are
    all ECDSA_OK has no eval error (its optimistic run was the reference's run); for any other one the
    error is tx.eval_rerun(lookup), used verbatim. lookup answers from the window's table; a triple the
    optimistic runs never asked for (OP_CHECKMULTISIG tries other pairs once one fails) is verified in a
    further call. Any non-zero status is false (verify.rs:60-67: unwrap_or(false))."""
    checks = [c for tx in txs for c in tx.ecdsa_checks]
    if not checks:
        return lambda tx: None
    if verify_ecdsa is None:
        if ctx is None:
            raise zg.ZgError(-1, "transactions carry ECDSA checks but no ECDSA backend was given "
                                 "(pass ctx= or verify_ecdsa=)")
        verify_ecdsa = ctx.ecdsa_verify
    keys = [(bytes(c.pubkey), bytes(c.sig), bytes(c.sighash)) for c in checks]
    sts = verify_ecdsa([k[0] for k in keys], [k[1] for k in keys], [k[2] for k in keys])
    table = {k: st == zg.ECDSA_OK for k, st in zip(keys, sts)}

    def lookup(pubkey, sig, sighash):
        k = (bytes(pubkey), bytes(sig), bytes(sighash))
        if k not in table:
            table[k] = verify_ecdsa([k[0]], [k[1]], [k[2]])[0] == zg.ECDSA_OK
        return table[k]

    where = {id(tx): i for i, tx in enumerate(txs)}

    def eval_error(tx):
        if all(table[(bytes(c.pubkey), bytes(c.sig), bytes(c.sighash))] for c in tx.ecdsa_checks):
            return None
        if tx.eval_rerun is None:
            raise zg.ZgError(-1, "a transaction's ECDSA check failed but it carries no eval_rerun")
        if not tx.ecdsa_requests:
            return tx.eval_rerun(lookup)

        def lookup_request(*key):
            """(pubkey, sig, sighash), or (input_index, pubkey, sig, script_code, hashtype) of a request"""
            if len(key) == 3:
                return lookup(*key)
            input_index, pubkey, sig, script_code, hashtype = key
            return lookup(pubkey, sig, resolve(where[id(tx)], input_index, script_code, hashtype))
        return tx.eval_rerun(lookup_request)
    return eval_error


def _input_errors(txs, ctx, inputs_verify, script_flags):
    """-> {window index: eval error or None} of the transactions that carry prevouts. Every input of theirs goes
    through ONE inputs_verify(raws, branch_ids, items, flags) call (default ctx.inputs_verify); a transaction's
    error is ("Signature", index, name) of its lowest failing input (TransactionEval::check walks the inputs in
    order, accept_transaction.rs:363-422), name the interpreter's error. An input that comes back without a
    verdict (not a template, out of range, a transaction the GPU does not parse) raises: it is the caller's."""
    need = [i for i, tx in enumerate(txs) if tx.prevouts is not None]
    for i in need:
        tx = txs[i]
        if tx.raw is None or tx.branch_id is None:
            raise ValueError("transaction %d carries prevouts but no raw bytes or no branch id" % i)
        if tx.ecdsa_checks or tx.ecdsa_requests or tx.eval_rerun is not None:
            raise ValueError("transaction %d carries prevouts and ecdsa_checks, ecdsa_requests or eval_rerun: "
                             "a transaction of template inputs has no interpreter run" % i)
    if not need:
        return {}
    if inputs_verify is None:
        if ctx is None:
            raise zg.ZgError(-1, "transactions carry prevouts but no backend was given (pass ctx= or inputs_verify=)")
        inputs_verify = ctx.inputs_verify
    items = [(k, j, bytes(p.script_pubkey), p.amount) for k, i in enumerate(need) for j, p in enumerate(txs[i].prevouts)]
    res = inputs_verify([bytes(txs[i].raw) for i in need], [txs[i].branch_id for i in need], items, script_flags)
    errors = {i: None for i in need}
    for (k, j, _, _), st in zip(items, res[1]):
        i = need[k]
        if st not in (zg.INPUT_OK,) + tuple(zg.INPUT_ERRORS):
            raise zg.ZgError(-1, "transaction %d: input %d was not verified (ZG_INPUT status %d); run its script on "
                                 "the host" % (i, j, st))
        if st != zg.INPUT_OK and errors[i] is None:
            errors[i] = ("Signature", j, zg.INPUT_ERRORS[st])
    return errors


def _shielded_verdicts(txs, ctx, shielded_verify, phgr=False):
    """-> {window index: (SHTX_* status, index)} of the transactions marked shielded, from ONE
    shielded_verify(raws, branch_ids) call for the window (default ctx.shielded_verify). A transaction the GPU gives no
    verdict on (PHGR JoinSplits, malformed or non-canonical bytes) raises: it is the caller's. phgr: the call is made
    with phgr=True (ZG_SHIELDED_PHGR), and a v2 / v3 transaction with JoinSplits has its verdict from it."""
    need = [i for i, tx in enumerate(txs) if tx.shielded]
    for i in need:
        tx = txs[i]
        if tx.raw is None or tx.branch_id is None:
            raise ValueError("transaction %d is marked shielded but carries no raw bytes or no branch id" % i)
        if (tx.joinsplits or tx.spends or tx.outputs or tx.js_pubkey is not None or tx.js_sig is not None
                or tx.binding_sig is not None or tx.sighash is not None):
            raise ValueError("transaction %d is marked shielded and carries proof or signature fields: its JoinSplit "
                             "and Sapling stage is read from its bytes" % i)
    if not need:
        return {}
    if shielded_verify is None:
        if ctx is None:
            raise zg.ZgError(-1, "transactions are marked shielded but no backend was given (pass ctx= or "
                                 "shielded_verify=)")
        shielded_verify = ctx.shielded_verify
    kw = {"phgr": True} if phgr else {}
    res = shielded_verify([bytes(txs[i].raw) for i in need], [txs[i].branch_id for i in need], **kw)
    out = {}
    for k, i in enumerate(need):
        st = res[1][k]
        if st not in (zg.SHTX_OK, zg.SHTX_NONE) + tuple(zg.SHTX_ERRORS):
            raise zg.ZgError(-1, "transaction %d: the shielded stage was not verified (ZG_SHTX status %d); check it "
                                 "on the host" % (i, st))
        out[i] = (st, res[2][k])
    return out


def _shielded_error(tx, verdict):
    """the JoinSplit and Sapling stage of a transaction marked shielded: the GPU's first error with the caller's
    outcomes at their places (accept_transaction.rs:575-596,649-657,737-741)"""
    st, index = verdict
    if st == zg.SHTX_JOINSPLIT_SIGNATURE:
        return "JoinSplitSignature"
    tree = next(((i, e) for i, e in enumerate(tx.tree_errors) if e), None)
    if st == zg.SHTX_INVALID_JOINSPLIT and (tree is None or index <= tree[0]):
        return ("InvalidJoinSplit", index)
    if tree is not None:
        return tree[1]
    if tx.js_nullifier_error:
        return tx.js_nullifier_error
    if st == zg.SHTX_INVALID_SAPLING:
        return "InvalidSapling"
    return tx.sapling_nullifier_error


def _tx_error(tx, plan, status, sp_ok=None, bind_ok=None, pghr_status=(), js_sig_ok=None, eval_error=None,
              input_error=None, shielded=None):
    """the reference's first error of one transaction, given the proof statuses; eval_error(tx) is asked
    only when no earlier check failed. input_error: the eval error of a transaction of template inputs;
    shielded: the (status, index) of a transaction marked shielded"""
    if js_sig_ok is None:
        js_sig_ok = tx.js_sig_ok
    js_plan, sp_plan, out_plan = plan
    if sp_ok is None:
        sp_ok = [s.sig_ok for s in tx.spends]
    if bind_ok is None:
        bind_ok = tx.binding_ok
    if tx.pre_error:
        return tx.pre_error
    if input_error is not None:
        return input_error
    if eval_error is not None and tx.ecdsa_checks:
        err = eval_error(tx)
        if err is not None:
            return err
    if shielded is not None:
        return _shielded_error(tx, shielded)
    if tx.joinsplits:
        if not js_sig_ok:
            return "JoinSplitSignature"
        for i, (d, (how, v)) in enumerate(zip(tx.joinsplits, js_plan)):
            ok = v if how == "caller" else (pghr_status[v] if how == "pghr" else status[v]) == OK
            if not ok:
                return ("InvalidJoinSplit", i)
            if d.tree_error:
                return d.tree_error
        if tx.js_nullifier_error:
            return tx.js_nullifier_error
    if tx.spends or tx.outputs:
        for ok, (how, v) in zip(sp_ok, sp_plan):
            if how == "prep" or not ok or status[v] != OK:
                return "InvalidSapling"
        for how, v in out_plan:
            if how == "prep" or status[v] != OK:
                return "InvalidSapling"
        if not bind_ok:
            return "InvalidSapling"
        if tx.sapling_nullifier_error:
            return tx.sapling_nullifier_error
    return None


def _chunked(verify, cap):
    """an import window larger than one batch (the context's max_batch) is verified as
    consecutive batches of at most `cap` proofs; statuses are joined in order (per-proof
    statuses do not depend on how proofs are grouped into batches)"""
    if not cap:
        return verify

    def run(proofs, kinds, inputs, n_inputs):
        n = len(kinds)
        out = []
        for lo in range(0, n, cap):
            hi = min(n, lo + cap)
            out += list(verify(proofs[192 * lo:192 * hi], kinds[lo:hi], inputs[zg.INPUT_STRIDE * lo:zg.INPUT_STRIDE * hi],
                               n_inputs[lo:hi]))
        return out
    return run


def verify_block(txs, verify=None, ctx=None, verify_sigs=None, sapling_bvk=None, verify_pghr=None,
                 verify_js_sigs=None, verify_ecdsa=None, sighash=None, inputs_verify=None,
                 script_flags=zg.SCRIPT_VERIFY_DERSIG, shielded_verify=None, shielded_phgr=False):
    """Check the shielded proofs of a block (or an import window: a flat list of Tx in chain
    order). Returns None if every transaction passes, else (tx_index, error) with the error the
    reference reports (accept_chain.rs:79-80: the lowest failing index wins).

    verify(proofs, kinds, inputs, n_inputs) -> statuses; default: ctx.verify_batch (ONE GPU
    batch for the whole block, exact per-proof statuses via bisection). A window larger than
    the context's max_batch (or a `verify.max_batch` attribute) is split into consecutive
    batches. Transactions that carry their sighash get their RedJubjub signatures verified on
    the GPU too (verify_sigs / sapling_bvk default to ctx.redjubjub_verify / ctx.sapling_bvk).
    PHGR JoinSplit proofs go through verify_pghr(proofs, inputs) -> statuses, default
    ctx.pghr13_verify (ONE zg_pghr13_verify call for the window). Transactions that carry their
    JoinSplit signature (Tx.js_sig, with js_pubkey and sighash) get it verified through
    verify_js_sigs(pubkeys, sigs, msgs) -> ED_* statuses, default ctx.ed25519_verify (ONE
    zg_ed25519_verify call for the window); the others keep the caller's js_sig_ok. The recorded
    ECDSA checks of the transparent inputs (Tx.ecdsa_checks) go through verify_ecdsa(pubkeys, sigs,
    msgs) -> ECDSA_* statuses, default ctx.ecdsa_verify (ONE zg_ecdsa_verify call for the window); the
    eval error of a transaction with a failed check is its eval_rerun's, placed after pre_error and
    before the JoinSplit and Sapling stages (accept_transaction.rs:68-84). Transactions that carry their
    serialized bytes (Tx.raw, Tx.branch_id) get the sighashes they lack -- the no-input one, and one per
    Tx.ecdsa_requests entry -- from sighash(raws, branch_ids, items) -> (tx statuses, hashes, statuses),
    default ctx.sighash (ONE zg_sighash call for the window, before the signature batches); a transaction
    the GPU reports as malformed or non-canonical raises ZgError and is the caller's to hash. Transactions whose
    inputs are all templates (Tx.prevouts) have every input verified through inputs_verify(raws, branch_ids, items,
    flags) -> (tx statuses, statuses, ...), default ctx.inputs_verify (ONE zg_inputs_verify call for the window, made
    with script_flags: bip66_height is 0 on every network); their eval error stands where eval_rerun's does, and an
    input the GPU gives no verdict on raises ZgError. Transactions marked Tx.shielded have their whole JoinSplit and
    Sapling stage read from their bytes through shielded_verify(raws, branch_ids) -> (tx statuses, SHTX_* statuses,
    indices, ...), default ctx.shielded_verify (ONE zg_shielded_verify call for the window); the caller's tree_errors
    and nullifier errors keep their places around its verdict, and a transaction it gives no verdict on raises
    ZgError. With shielded_phgr that one call is made with phgr=True (ZG_SHIELDED_PHGR) and a
    marked v2 / v3 transaction with PHGR JoinSplits is accepted: its Ed25519 signature and PGHR13 proofs are checked
    in the call; without it such a transaction raises ZgError as before. Without the mark nothing changes."""
    input_errors = _input_errors(txs, ctx, inputs_verify, script_flags)
    shielded = _shielded_verdicts(txs, ctx, shielded_verify, shielded_phgr)
    txs, resolve = _resolve_sighashes(txs, ctx, sighash)
    items, pghr, plans = _queue(txs, ctx)
    if verify is None:
        def verify(proofs, kinds, inputs, n_inputs):
            return ctx.verify_batch(proofs, kinds, inputs, n_inputs)[0]
        cap = getattr(ctx, "max_batch", None)
    else:
        cap = getattr(verify, "max_batch", None)
    verify = _chunked(verify, cap)
    status = []
    if items:
        proofs = b"".join(p for _, p, _, _ in items)
        kinds = bytes(k for k, _, _, _ in items)
        inputs = b"".join(row for _, _, row, _ in items)
        n_inputs = bytes(nin for _, _, _, nin in items)
        status = list(verify(proofs, kinds, inputs, n_inputs))
    pghr_status = []
    if pghr:
        if verify_pghr is None:
            if ctx is None:
                raise zg.ZgError(-1, "PHGR JoinSplits in the window but no PGHR13 backend (pass ctx= or verify_pghr=)")
            verify_pghr = ctx.pghr13_verify
        pghr_status = list(verify_pghr([p for p, _ in pghr], [inp for _, inp in pghr]))
    sp_ok, bind_ok = _sig_verdicts(txs, ctx, verify_sigs, sapling_bvk)
    js_ok = _js_sig_verdicts(txs, ctx, verify_js_sigs)
    eval_error = _eval_errors(txs, ctx, verify_ecdsa, resolve)
    for idx, (tx, plan) in enumerate(zip(txs, plans)):
        err = _tx_error(tx, plan, status, sp_ok[idx], bind_ok[idx], pghr_status, js_ok[idx], eval_error,
                        input_errors.get(idx), shielded.get(idx))
        if err is not None:
            return idx, err
    return None
