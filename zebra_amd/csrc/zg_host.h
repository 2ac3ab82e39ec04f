// zg_host.h -- the host state shared by the units behind the C ABI that hold a context (zg.hip,
// zg_calls.hip): zg_hostkit.h, and over it zg_dev, zg_ctx and what goes with them. Host code only,
// and no kernel.
#pragma once
#include "zg_hostkit.h"
#include "zg_blake2b.h"
#include "zg_msm.h"  // MsmBufs; RawVK, DevVK and the point and field types come with it

namespace zg {
// BLAKE2b-outlen(tag || le64(seed) || le64(i)): what seeded contexts (tests) and the synthetic
// workload derive their scalars from
inline void seeded_bytes(const char* tag, uint64_t seed, uint64_t i, uint8_t* out, size_t outlen) {
  Blake2b h(outlen);
  h.update(tag, strlen(tag));
  uint8_t le[16];
  for (int b = 0; b < 8; b++) {
    le[b] = (uint8_t)(seed >> (8 * b));
    le[8 + b] = (uint8_t)(i >> (8 * b));
  }
  h.update(le, 16);
  h.final(out);
}
}  // namespace zg

#define ZG_LP_PARTS_MAX 8
#define ZG_NEV (16 + ZG_LP_PARTS_MAX)  // [13]: zg_gt_check; [14..] line-product parts, [14 + max] chains done,
                                       // [15 + max] settle_batch (no timing)
#define ZG_NTIMINGS 9
#define ZG_NSTATS 13
#define ZG_TREE_COOP_BELOW 4096  // product-tree levels with fewer nodes run one wave per node
#define ZG_K4_MIN 16384          // lone batches from this many (padded) proofs sum r_i C_i by K4's Pippenger
                                 // buckets; smaller lone batches by the GLV products in decode + the C tree
                                 // levels (run_pipeline: batches in flight always use K4)
#define ZG_PGHR_CHUNK 65536      // proofs per batch check of zg_pghr13_verify (ZG_PGHR_CHUNK lowers it, 64 at the least)
#define ZG_TXID_HOST_MIN 65536   // slices from this many bytes are hashed on host threads beside k_txid: a 100 KB
                                 // transaction in a 65,536-transaction window, 15.5 -> 9.8 ms per call
#define ZG_HI_PAIRS 4            // high-priority stream pairs per device (zg_set_priority round-robin)

// Per-device state shared by every context (batch slot) on that GPU: a FIXED pool of stream
// pairs, created once, and the prepared verifying keys. A context only owns buffers, so a
// process can hold any number of slots without creating another HIP stream / hardware queue.
// Why: each hardware queue that dispatches a kernel with a private (scratch) segment keeps a
// scratch allocation sized for the whole device; the process's scratch pool is bounded, and
// with a stream pair per context the 7th in-flight context on one GPU pushed it over
// (HSA_STATUS_ERROR_OUT_OF_RESOURCES from the queue). With the pool, the
// number of queues -- hence of scratch reservations -- no longer grows with the slots.
struct zg_dev {
  int device = 0;
  int ncu = 0;
  int refs = 0;
  std::mutex mu;  // the pool cursor and the VK cache
  int npairs = 0;
  hipStream_t main[16] = {}, side[16] = {};
  // high-priority pairs (lazy, zg_set_priority): a few, so that concurrent checker contexts (one per
  // verdict thread) do not serialise their final exponentiations on one stream
  hipStream_t hi_main[ZG_HI_PAIRS] = {}, hi_side[ZG_HI_PAIRS] = {};
  int hi_next = 0;
  int next = 0;
  struct VKEntry {
    zg::RawVK raw;
    zg::DevVK* d = nullptr;
    uint32_t* comb = nullptr;  // the key's comb tables (ZG_COMB_POINTS x 96 B, k_vk_comb)
    int err = 0;
  };
  std::vector<VKEntry*> vks;  // prepare_verifying_key once per distinct key per device
  uint32_t* jj_comb = nullptr;  // Jubjub generators' comb tables (zg_jubjub.h), built on first use
  uint32_t* ed_comb = nullptr;  // the Ed25519 base point's comb table (zg_ed25519.h), built on first use
  uint32_t* ec_comb = nullptr;  // the secp256k1 generator's comb table (zg_ecdsa.h), built on first use
  zg::MerkleDev* merkle = nullptr;  // Pedersen table + empty roots (zg_merkle.hip), first use
  zg::BnDev* bn = nullptr;          // PGHR13 key, line and comb tables (zg_pghr13.hip), first use
  std::atomic<int> inflight{0};     // contexts on this device with a batch begun and not finished
};

struct zg_ctx {
  int device = 0;
  zg_dev* dev = nullptr;
  hipStream_t stream = nullptr;  // from the device pool (not owned)
  hipStream_t side = nullptr;    // VK-side root work, concurrent with the Miller kernels
  int pair = 0;
  std::mutex mu;
  std::string err;
  uint32_t cap = 0;  // power of two >= max_batch
  int seeded = 0;
  uint64_t seed = 0;
  int vk_loaded[ZG_NKINDS] = {0, 0, 0};
  int vk_iclen[ZG_NKINDS] = {0, 0, 0};
  zg::RawVK vk_raw[ZG_NKINDS];  // host copies of the loaded keys (shared alpha / beta / gamma test)
  int merged = 0;           // loaded keys share alpha, beta, gamma: merged VK-side pairs (zg_batch.h)
  zg::DevVK* d_vk = nullptr;  // this slot's 3 kinds (copied from the device cache)
  int* d_int = nullptr;   // scratch ints: [8] bfail, [9] fused-wait failure
  // batch
  uint8_t *d_proofs = nullptr, *d_kinds = nullptr, *d_inputs = nullptr, *d_ninputs = nullptr, *d_r = nullptr,
          *d_status = nullptr, *d_bytes = nullptr, *d_okbits = nullptr;
  zg::G1A* d_ptA = nullptr;
  zg::G1A* d_ptAC = nullptr;
  int* d_prog = nullptr;  // cap / 64: per lines block, steps published (fused R-chain + f-chain)
  int ncu = 0;            // compute units of the device
  int fuse = -1;          // ZG_LINES_FCHAIN: -1 auto (both grids resident at once), 0 never, 1 always
  int fuse_off = 0;       // a fused launch ever timed out waiting: split launches from then on
  int serial_side = 0;    // ZG_SERIAL_SIDE=1: the side-stream work runs on the main stream after the
                          // product tree (measurement: the Miller kernels alone on the device)
  zg::G2A* d_ptB = nullptr;
  zg::Fq12* d_ftree = nullptr;
  zg::Fq2* d_lines = nullptr;  // cap x 68 x 3: per-proof line triples (R-chain -> f-chain)
  zg::Fq2* d_lprod = nullptr;  // cap / 4 x 68 x 6: per-group line products (k_line_prod)
  zg::Fq2* d_fstate = nullptr; // cap / 4 x 6: each group chain's f between its parts (k_batch_fchaing)
  zg::G1J* d_ctree = nullptr;
  zg::Fr* d_stree = nullptr;
  zg::MsmBufs msm = {};       // K4: Pippenger sum r_i C_i per key + root Fr sums (zg_msm.h)
  int trees_built = 0;    // the full C / Fr trees exist for this batch (bisection only)
  int c_tree_pending = 0; // the C tree is still being built on the side stream (ev[12])
  // node checks
  int* d_nodes = nullptr;
  zg::G1J* d_msm = nullptr;
  zg::Fq12* d_pairf = nullptr;
  int* d_ok = nullptr;
  zg::Fq12* d_out = nullptr;
  // state of the split API
  int state = 0;
  size_t n = 0, npad = 0;
  const uint8_t* cur_ninputs = nullptr;  // device pointer or null
  // this batch's inputs on the device: the context's own buffers (host-buffer calls copy into
  // them), or the caller's HBM-resident buffers (zg_batch_begin_device: read in place, no copy)
  const uint8_t *cur_proofs = nullptr, *cur_kinds = nullptr, *cur_inputs = nullptr;
  int root_pairs_ready = 0;  // the pipeline already ran the root's MSM + VK pairs on `side`
  int settled = 0;           // settle_batch ran for this batch
  int alone_last = 0;        // the last batch ran with no other batch in flight (K4 shape)
  int eager = 0;             // the pipeline's last steps copied the root partial, flags and statuses to h_pin (ev[4])
  uint8_t* h_pin = nullptr;  // pinned host memory: ZG_PIN_* layout
  uint8_t* h_gt = nullptr;   // pinned staging of zg_gt_check (partials in, verdict out; grow-only)
  size_t h_gt_cap = 0;
  int fused_last = 0;        // the last batch used the fused R-chain + f-chain launch
  int lines_lane = -1;      // ZG_LINES_LANE: -1 auto (the straight-line R-chain from ZG_LINES_LANE_MIN padded
                            // proofs, sized for 1 wave per SIMD when the batch is alone on the device, else
                            // 2; the staged program below), 1 / 2 always straight-line sized for 2 / 1
                            // waves per SIMD, 0 always the staged program (zg_kernels.h)
  int quads = -1;            // ZG_FCHAIN_QUADS: -1 auto (npad >= ZG_QUAD_MIN), 0 never, 1 always (npad >= 4)
  int line_group = -1;       // ZG_LINE_GROUP: proofs per group (k_line_prod): -1 auto (32 from ZG_LINE_PROD_MIN
                             // padded proofs, else the quad chain), 0 never, a power of two >= 4 always
  int lineprod_last = 0;     // the last batch's f-chain ran on group line products (no tree below the groups)
  int lines_affine = 0;      // ZG_LINES_AFFINE: K (2, 4, 8) -- the group line products run on affine lines from
                             // k_batch_lines_aff, K proofs per lane (round 6); 0 projective
  int lines_affine_xl = 0;   // ZG_LINES_AFFINE_XL=1: its cross-lane variant (one inversion per wave; K = 4)
  int affine_last = 0;       // the last batch's lines are affine (bisection re-forms projective ones)
  int quad_split = 1;        // ZG_QUAD_SPLIT: 1 a step's four lines multiply first, then into f (Q4IK + GM / GMSQ,
                             // round 6), 0 the fused Q4 / Q4SQ programs (same values)
  int lp_parts = 0;          // ZG_LINE_PROD_PARTS: step parts overlapping line products and chains: 1..8 equal
                             // parts, 0 (default) wave-aligned parts (lineprod_parts)
  int glv_lds = ZG_DEC_GLV_LDS;  // ZG_DEC_GLV_LDS: decode's r_i A_i two columns per step from an LDS table, in a
                             // launch of its own (K4 layout only; zg_decode.h)
  int pairs_late = 0;        // ZG_PAIRS_LATE=1: with group line products, the root's VK MSM + pairs go on the side
                             // stream AFTER the group chains instead of before them (round 6, r06f: 8k with line
                             // products 2.88 -> 2.77 ms per batch, still behind the quad chain's 2.61; 16k 4.19 ->
                             // 4.30, 64k 12.33 -> 12.46: not the default)
  long k4_min = ZG_K4_MIN;   // ZG_K4_MIN overrides: K4 Pippenger from this many padded proofs, else decode GLV + C tree
  int k4_last = 1;           // the last batch summed r_i C_i with K4 (0: the C tree is built, bisection reuses it)
  int quads_last = 0;        // the last batch's f-chain ran four proofs per lane (no pair-level nodes)
  int singles = -1;          // ZG_FCHAIN_SINGLE: -1 auto (a fused launch runs one proof per f-chain lane), 0 never
  int singles_last = 0;      // the last batch's f-chain wrote the per-proof leaves (bisection reuses them)
  size_t coop_below = ZG_TREE_COOP_BELOW;  // ZG_TREE_COOP_BELOW overrides (product-tree wave-per-node levels)
  hipEvent_t ev[ZG_NEV] = {};
  float timings[ZG_NTIMINGS] = {};
  // [0] batches, [1] fused launches, [2] fused-wait failures, [3] B subgroup failures
  // (bfail, deferred recomputes), [4] bisections, [5] nodes checked by bisection,
  // [6] K4 bucket entries of the last batch (points with a non-zero digit, summed over windows)
  uint64_t stats[ZG_NSTATS] = {};
  uint64_t calls = 0;
  int debug_each = 0;         // ZG_DEBUG_EACH=1: every batch's statuses re-checked per proof
  uint8_t* d_dbg = nullptr;   // the per-proof statuses of that re-check
  const zg::BnKey* bn_key = nullptr;  // this slot's PGHR13 key (an immutable, reference-counted entry of the device cache)
  zg::DevScratch own;        // every d_* buffer above (zg_create); freed with the context
  zg::DevArena prep_arena;   // zg_prep_batch device buffers
  zg::DevArena tree_arena;   // zg_tree_roots scratch (zg_merkle.hip)
  zg::DevArena bn_arena;     // zg_pghr13_verify scratch (zg_pghr13.hip)
  zg::DevArena inputs_arena; // zg_inputs_verify device buffers
  zg::DevArena shielded_arena; // zg_shielded_verify device buffers
  // the launch shape of zg_pghr13_verify's batch check (zg_pghr13.hip bn_pghr13_shape; zg_pghr13_shape reports it)
  int pghr_straus_b = 0;     // ZG_STRAUS_B: proofs per lane of k_pghr_straus, 1 / 2 / 4; 0 (any other value) by size
  int pghr_bseg_k = 0;       // ZG_BSEG_K: proofs per lane of k_pghr_bseg, 1..32 (larger: 32); 0 (or less) by size
  size_t pghr_chunk = ZG_PGHR_CHUNK;  // ZG_PGHR_CHUNK: proofs per batch check of one call, 64..65,536
  size_t txid_host_min = ZG_TXID_HOST_MIN;  // ZG_TXID_HOST_MIN: slices of at least this many bytes are hashed on
                                            // host threads beside k_txid; 0: never
  hipEvent_t sig_ev[2] = {};  // around the kernel of the last signature call (zg_last_sig_kernel_ms), first use
  float sig_ms = 0.0f;
};

inline int fail(zg_ctx* c, int code, const std::string& msg) {
  c->err = msg;
  return code;
}

namespace zg {
// zg.hip, for zg_shielded_verify: zg_verify_batch over rows on the device, read in place as zg_batch_begin_device
// reads them (all three keys loaded, n <= max_batch); status on the host. The caller holds ctx->mu for the whole call
int batch_verify_device_locked(zg_ctx* ctx, size_t n, const uint8_t* d_proofs, const uint8_t* d_kinds,
                               const uint8_t* d_inputs, const uint8_t* d_n_inputs, uint8_t* status);
}  // namespace zg
