"""Import-window batching of block acceptance.

The reference imports blocks one at a time (sync/src/blocks_writer.rs:63-90): a block already
in storage is skipped; a block whose parent is unknown goes to the orphan pool (at most
MAX_ORPHANED_BLOCKS = 1024, else TooManyOrphanBlocks); otherwise the block and every orphan
descendant are verified in order and inserted, and the first verification error ends the call.
A real block carries few Groth16 proofs, so a GPU batch per block would be tiny.

DeferredBlocksWriter keeps exactly that observable behaviour -- the same blocks end up in
storage, in the same order, and the same first error is reported -- while the Groth16 proofs and
Sapling signatures of many consecutive blocks are verified together: each block's other checks
run when it is appended (against a pending view of the chain that already includes the blocks
appended before it), its proof-carrying transactions join a window, and the window is verified
with ONE zebra_amd.collector.verify_block call when it holds `window_proofs` proofs, when a
block's own checks fail (the blocks before it may hold an earlier error), or on flush(). Blocks
are inserted into storage only once their window has verified, in chain order, up to the first
failing block; that block's error is raised and the window's later blocks are dropped, just as
the sequential writer would never have inserted them.

Error precedence inside a block is the collector's (accept_transaction.rs:68-84,
accept_chain.rs:76-81: the lowest failing transaction wins); across blocks the lowest block wins.

Headers: a block that carries its 1487 serialized header bytes
(`Block.header`) has HeaderVerifier::check's Equihash and proof-of-work steps
(verification/src/verify_header.rs:26-32) deferred too: the headers of a window go through ONE
zg_headers_verify call when the window is verified, before the collector call. Per block the
order is the reference's: `header_precheck` (the version check, evaluated at append) ->
InvalidEquihashSolution -> Pow -> `precheck` (the timestamp and everything after it) ->
transactions. A block whose `precheck` fails at append still has its header verified with the
window it flushes, and a header error outranks its `precheck` error. With `header=None` nothing
changes.

Block bodies: a block that carries its whole serialization (`Block.raw`) has
BlockVerifier::check (verification/src/verify_block.rs:31-40: empty, coinbase, size, extra coinbases,
uniqueness, sigops, merkle root) deferred as well: the window's blocks that carry `raw` go through ONE
zg_blocks_verify call when the window is verified. Per block the order is the reference's
(verification/src/verify_chain.rs:35-42: block.check(), then the header, then the transactions): the
BlockVerifier error comes before that block's header error and before its transaction errors, and still
after a `header_precheck` failure raised at append. The writer keeps the transaction ids the call returns
(`txids[block.hash]`), so the caller need not hash again. With `raw=None` nothing changes.

Contract: the equivalence holds for a caller that stops at the first error, as the reference's
only caller does (zebra/commands/import.rs:20-28 returns on any Err from append_block). The
error of a block surfaces when its window is verified -- at that block's append_block or at a
later append_block / flush -- and the window's blocks after the failing one are dropped,
including blocks on a sibling fork that the sequential writer would have inserted had the caller
kept appending after the error. Forks inside a window are otherwise handled like the sequential
writer (tests/test_blocks_writer.py: sibling forks with and without failures).
"""
from collections import OrderedDict

from . import collector

MAX_ORPHANED_BLOCKS = 1024
MAINNET_MAX_BITS = 0x1f07ffff   # Network::Mainnet.max_bits() (network/src/network.rs:14,47-54) as a compact
# zg_headers_verify status -> the reference's error (verification/src/error.rs); a header whose solution
# does not deserialize never reaches the reference's writer
HEADER_ERRORS = {1: "MalformedHeader", 2: "InvalidEquihashSolution", 3: "Pow"}
# zg_blocks_verify status -> the reference's error; Size and the misplaced coinbase carry the call's detail
# word. A block that does not deserialize never reaches the reference's writer; a non-canonical one (the
# chain holds none) is reported as such
BLOCK_ERRORS = {1: "MalformedBlock", 2: "NoncanonicalBlock", 3: "Empty", 4: "Coinbase", 5: "Size",
                6: "MisplacedCoinbase", 7: "DuplicatedTransactions", 8: "MaximumSigops", 9: "MerkleRoot"}
MAINNET_MAX_BLOCK_SIZE = 2000000     # ConsensusParams::max_block_size (network/src/consensus.rs)
MAINNET_MAX_BLOCK_SIGOPS = 20000     # ConsensusParams::max_block_sigops


def block_error(status, detail):
    """Error::Size(size), Error::Transaction(index, MisplacedCoinbase), or the bare name"""
    name = BLOCK_ERRORS[status]
    return ("Size", detail) if status == 5 else ("Transaction", detail, name) if status == 6 else name


class WriterError(Exception):
    """sync::Error: kind is "TooManyOrphanBlocks" | "Verification" | "Database"."""

    def __init__(self, kind, detail=None):
        super().__init__("%s%s" % (kind, "" if detail is None else ": %r" % (detail,)))
        self.kind = kind
        self.detail = detail

    def __eq__(self, other):
        return isinstance(other, WriterError) and (self.kind, self.detail) == (other.kind, other.detail)

    def __hash__(self):
        return hash((self.kind, repr(self.detail)))


class Block:
    """an indexed block: its hash, its parent's hash and the collector view of its transactions.
    precheck(writer) -> None | error: the block's checks that precede every transaction
    acceptor (chain_verifier.rs:32-132: ChainVerifier::check -- header, block and the
    context-free transaction checks -- then BlockAcceptor / HeaderAcceptor), run against the chain
    as it will be once every block appended before this one is accepted. The transaction-level
    outcomes that are not proofs (scripts, tree roots, nullifiers, ...) are set on the collector
    Tx objects by the same caller."""

    def __init__(self, hash, parent, txs, precheck=None, header=None, header_precheck=None, raw=None):
        """raw: the whole serialized block, or None (the caller ran BlockVerifier::check itself, inside
        precheck); header: the 1487 serialized header bytes, or None (the caller ran HeaderVerifier::check itself,
        inside precheck); header_precheck(writer) -> None | error: the checks that precede the Equihash
        solution (HeaderVersion::check), run when the block is appended"""
        self.hash, self.parent, self.txs, self.precheck = hash, parent, txs, precheck
        self.header, self.header_precheck, self.raw = header, header_precheck, raw

    def n_proofs(self):
        return sum(len(t.joinsplits) + len(t.spends) + len(t.outputs) for t in self.txs)


class _OrphanPool:
    """OrphanBlocksPool (sync/src/utils/orphan_blocks_pool.rs): orphans by parent hash, insertion
    ordered; remove_blocks_for_parent returns every descendant, parents before children."""

    def __init__(self):
        self.by_parent = OrderedDict()

    def __len__(self):
        return sum(len(v) for v in self.by_parent.values())

    def insert(self, block):
        self.by_parent.setdefault(block.parent, OrderedDict())[block.hash] = block

    def remove_for_parent(self, h):
        out, queue = [], [h]
        while queue:
            p = queue.pop(0)
            kids = self.by_parent.pop(p, None)
            if kids:
                for b in kids.values():
                    out.append(b)
                    queue.append(b.hash)
        return out


class SequentialBlocksWriter:
    """BlocksWriter::append_block as the reference runs it: every block verified on its own as
    it is appended (check(block) -> None | error), then inserted."""

    def __init__(self, storage, check):
        self.storage, self.check, self.orphans = storage, check, _OrphanPool()

    def append_block(self, block):
        if self.storage.contains(block.hash):
            return
        if not self.storage.contains(block.parent):
            self.orphans.insert(block)
            if len(self.orphans) > MAX_ORPHANED_BLOCKS:
                raise WriterError("TooManyOrphanBlocks")
            return
        for b in [block] + self.orphans.remove_for_parent(block.hash):
            err = self.check(b)
            if err is not None:
                raise WriterError("Verification", err)
            self.storage.insert(b)

    def flush(self):
        return None


class DeferredBlocksWriter:
    """The same behaviour with the proofs of a window verified in one batch.

    verify_window(txs) -> None | (tx_index, error): the collector over the window's flattened
    transactions (default: collector.verify_block with `ctx`, i.e. one GPU batch).
    verify_headers(headers) -> list of HDR_* statuses: the window's headers in one call (default:
    ctx.headers_verify against the compact `max_bits`, the network's proof-of-work limit).
    verify_blocks(raws) -> (list of BLK_* statuses, list of detail words, list of id lists): the window's
    serialized blocks in one call (default: ctx.blocks_verify against `max_block_size` / `max_block_sigops`)."""

    def __init__(self, storage, ctx=None, verify_window=None, window_proofs=65536, verify_headers=None,
                 max_bits=MAINNET_MAX_BITS, window_headers=16384, verify_blocks=None,
                 max_block_size=MAINNET_MAX_BLOCK_SIZE, max_block_sigops=MAINNET_MAX_BLOCK_SIGOPS):
        self.storage = storage
        self.orphans = _OrphanPool()
        self.window = []          # pending blocks in chain order (prechecked, not inserted)
        self.pending = set()      # their hashes: children may build on them
        self.window_proofs = window_proofs
        if verify_window is None:
            def verify_window(txs):
                return collector.verify_block(txs, ctx=ctx)
        self.verify_window = verify_window
        self.window_headers = window_headers
        if verify_headers is None:
            def verify_headers(headers):
                if ctx is None:
                    raise RuntimeError("a block carries its header but the writer has neither a context "
                                       "nor verify_headers")
                return ctx.headers_verify(headers, max_bits)[0]
        self.verify_headers = verify_headers
        if verify_blocks is None:
            def verify_blocks(raws):
                if ctx is None:
                    raise RuntimeError("a block carries its serialization but the writer has neither a context "
                                       "nor verify_blocks")
                st, _, detail, _, _, ids = ctx.blocks_verify(raws, max_block_size, max_block_sigops)
                return st, detail, ids
        self.verify_blocks = verify_blocks
        self.txids = {}           # block hash -> its transaction ids, of the blocks whose body was verified here

    def _known(self, h):
        return h in self.pending or self.storage.contains(h)

    def append_block(self, block):
        if self._known(block.hash):
            return
        if not self._known(block.parent):
            self.orphans.insert(block)
            if len(self.orphans) > MAX_ORPHANED_BLOCKS:
                self.flush()               # blocks appended before keep their verdicts first
                raise WriterError("TooManyOrphanBlocks")
            return
        for b in [block] + self.orphans.remove_for_parent(block.hash):
            hpre = b.header_precheck(self) if b.header is not None and b.header_precheck else None
            if hpre is not None:
                # fails before its Equihash solution is looked at: only earlier blocks can precede it
                self.flush()
                raise WriterError("Verification", hpre)
            pre = b.precheck(self) if b.precheck else None
            if pre is not None:
                # the block fails before its transactions are accepted; an earlier block of the
                # window may hold the first error: verify (and accept) those first -- with this
                # block's header, whose Equihash / Pow error comes before `pre`
                self.flush(_tail=b if b.header is not None or b.raw is not None else None)
                raise WriterError("Verification", pre)
            self.window.append(b)
            self.pending.add(b.hash)
            if sum(x.n_proofs() for x in self.window) >= self.window_proofs or \
                    sum(x.header is not None for x in self.window) >= self.window_headers:
                self.flush()

    def flush(self, _tail=None):
        """verify the window, insert its blocks up to the first failing one, raise its error.
        _tail: a block that already failed its precheck and is not part of the window; its header is
        verified with the window's (a header error of it is raised here, after the window's own)"""
        if not self.window and _tail is None:
            return
        blocks = self.window
        # the headers first, ONE call: the first failing header bounds what else can matter
        seq = blocks + ([_tail] if _tail is not None else [])
        # the bodies, ONE call; a block's BlockVerifier error comes before its header error
        with_raw = [i for i, b in enumerate(seq) if b.raw is not None]
        bfail, berr, ids = len(seq), None, {}
        if with_raw:
            sts, details, idlists = self.verify_blocks([seq[i].raw for i in with_raw])
            assert len(sts) == len(with_raw)
            for k, i in enumerate(with_raw):
                if sts[k] != 0:
                    bfail, berr = i, block_error(sts[k], details[k])
                    break
                ids[seq[i].hash] = idlists[k]
        with_header = [i for i, b in enumerate(seq) if b.header is not None]
        hfail, herr = len(seq), None
        if with_header:
            sts = self.verify_headers([seq[i].header for i in with_header])
            assert len(sts) == len(with_header)
            for i, st in zip(with_header, sts):
                if st != 0:
                    hfail, herr = i, HEADER_ERRORS[st]
                    break
        if bfail <= hfail and berr is not None:
            hfail, herr = bfail, berr
        flat, owner = [], []
        for bi, b in enumerate(blocks[:hfail]):
            for ti, t in enumerate(b.txs):
                flat.append(t)
                owner.append((bi, ti))
        # verify BEFORE the window is taken: a backend failure (GPU error) raises with the window
        # and the pending set unchanged, so the caller can retry or re-run it on another backend
        res = self.verify_window(flat) if flat else None
        self.window, self.pending = [], set()
        self.txids.update(ids)
        fail_block = len(blocks)
        err = None
        if res is not None:
            idx, e = res
            fail_block, ti = owner[idx]
            err = (ti, e)
        elif herr is not None:
            # (every transaction in `flat` belongs to a block before hfail: a transaction error wins)
            fail_block, err = min(hfail, len(blocks)), herr
        for b in blocks[:fail_block]:
            self.storage.insert(b)
        if err is not None:
            raise WriterError("Verification", err)


class MemoryStorage:
    """storage::Store stand-in (db::BlockChainDatabase::init_test_chain on MemoryDatabase)"""

    def __init__(self, genesis_hash):
        self.blocks = [genesis_hash]
        self.set = {genesis_hash}

    def contains(self, h):
        return h in self.set

    def insert(self, block):
        assert block.parent in self.set, "inserted before its parent"
        self.blocks.append(block.hash)
        self.set.add(block.hash)
