// fused.hip -- the fused Llama decode step (crabml_hip_llama_*): the hot path as 5 kernels per layer, replayed from one
// hipGraph with token id / position resident in device memory, plus the batched prefill.  This file is the HOST side
// (context, segment enqueue, graph capture, C entry points); the kernels live in fused_common.hpp (quantizer lanes,
// norm, q/k/v), fused_attention.hpp and fused_ffn.hpp (wo / ffn_down with the norm epilogue, gate/up, sampler).
//
// It serves exactly the op sequence Llama2Runner<T> issues for one token (crabml-llama2/src/llama2.rs):
//   forward_llama :213-281, forward_multi_query_attention :527-603, forward_ffn :605-638, classifier :184-211
// with the reference's arithmetic (each fused stage cites the primitive it folds in).  Why fuse: the per-op
// trait path is launch-bound (31 launches/layer, GPU busy 1/3 of the time; profiles/r01_trait_path_kernel_
// trace.md).  The GEMV stages use the same lane-per-block / R-rows-per-wave mapping as gemv.hip and stay
// HBM-bound; the small stages are folded into their producers/consumers so activations never round-trip
// through extra launches:
//   k_norm_quant   rms_norm_inplace + mul_inplace(weight) + quantize_f32_q8_0        (1 workgroup)
//   k_qkv          wq/wk/wv matmul_vec + rope_inplace(q,k) + scale_inplace(q) + concatenate(k,v -> KV cache)
//   k_attn         batch_matmul(q,K^T) + softmax_inplace + batch_matmul(p,V) [+ quantize for wo]
//   k_gemv_res     wo / ffn_down matmul_vec + add_inplace(residual)
//   k_gateup       ffn_gate/ffn_up matmul_vec + silu_inplace + mul_inplace
//   k_argmax_step  greedy sampler (last maximum) + token/position advance
//   k_sample_*     temperature / top-p sampler + advance (sampler.hpp; crabml_hip_llama_decode_sample)
//
// Which instantiation a context launches, with which grid and how much LDS, is decided once and read by both llama_create_impl
// (which checks that the LDS fits and raises the kernels' limits) and the enqueue code: chunk_split (workgroups per chunk of wo /
// ffn_down), norm_nit, the *_lds_bytes functions beside their kernels, and the *_kernel selectors that hand out the function pointer
// of every kernel whose limit is raised.  with_const / with_const_else (kernels.hpp) turn a run-time value into the template argument, so a launch's
// argument list is written once; test_hook (common.hpp) is what arms an A/B or tuning hook.
// Which launches a context runs at all -- the segment path, its ordered form, the segment forms and the attention forms -- is decided once,
// by decide_step at create, as one value (StepPlan, c->plan); crabml_hip_debug_step_plan (crabml_hip_debug.h) reads it out for any
// configuration, on the record-only test device too, and tests/test_step_plan.py / tests/test_hip_step_plan.py hold the table.
#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>

#include "fused_common.hpp"
#include "fused_attention.hpp"
#include "fused_ffn.hpp"
#include "sampler.hpp"
#include "prefill_rows.hpp"
#include "lazy.hpp"


// ==============================================================================================================
// Host side: the decode step as a list of segments.  With tensor parallelism (tp_size > 1) every segment ends
// in a partial-sum vector that is all-reduced across ranks (RCCL over xGMI; 2 x dim f32 per layer):
//   segment 2l   : [embed] attn-norm(+ pending residual) -> qkv(local heads) -> attention -> wo(local k-slice)
//   segment 2l+1 : ffn-norm(+ pending residual) -> gate/up(local rows) -> down(local k-slice)
//   segment 2L   : final norm(+ pending residual) -> classifier -> greedy argmax / advance
// Column-parallel: wq/wk/wv by heads, gate/up by rows.  Row-parallel: wo, ffn_down by k.
// ==============================================================================================================
#include <dlfcn.h>

using namespace crabml_hip;

// ---- RCCL, bound at run time (the single-GPU product path never needs it) ------------------------------------
struct crabml_hip_tp_comm {
  crabml_hip_device* dev = nullptr;
  void* nccl = nullptr;  // ncclComm_t (RCCL kind)
  int nranks = 1, rank = 0;
  // P2P kind (crabml_hip_tp_p2p_*): the one-shot all-reduce over peer-mapped inboxes (fused_ffn.hpp, TpP2P)
  bool p2p = false;
  bool connected = false;
  unsigned long long* inbox = nullptr;   // this rank's inbox: TP_SLOTS slots x nranks rows x cap granules
  bool via_ipc[8] = {false};             // peer[r] was mapped with hipIpcOpenMemHandle (closed at destroy; plain pointers are not)
  size_t inbox_bytes = 0;
  unsigned cap = 0;                      // granules per row
  bool finegrained = false;
  void* peer[8] = {nullptr};             // peers' inboxes as mapped here (peer[rank] = inbox)
  int* fault = nullptr;                  // device word raised by a poll that timed out
  unsigned host_epoch = 0;               // crabml_hip_tp_all_reduce outside a decode step
  unsigned sessions = 0;                 // decode contexts created on this group so far (every rank creates them in the same order)
};
namespace {
struct NcclId {  // ncclUniqueId: 128 opaque bytes, passed BY VALUE to ncclCommInitRank
  char b[128];
};
struct Rccl {
  typedef NcclId IdT;
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.lib) break;
    }
    if (r.lib) {
      r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
      r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
      r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
      r.AllReduce = (decltype(r.AllReduce))dlsym(r.lib, "ncclAllReduce");
      r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
    }
  }
  return (r.lib && r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllReduce) ? &r : nullptr;
}
}  // namespace

// A parity tap: while armed for a layer, the enqueue code puts device-to-device copies of that layer's buffers between its launches
// (copy) and notes the launch plan where it decides it (note); the hook's entry point reads both back (export_fields).  Disarmed,
// copy and note do nothing, so the enqueue code calls them unconditionally.
struct TapRec {
  static constexpr int FIELDS = CRABML_HIP_PFTAP_FIELDS > CRABML_HIP_TAP_FIELDS ? CRABML_HIP_PFTAP_FIELDS : CRABML_HIP_TAP_FIELDS;
  static constexpr int WORDS = CRABML_HIP_PFTAP_PLAN_WORDS > CRABML_HIP_TAP_PLAN_WORDS ? CRABML_HIP_PFTAP_PLAN_WORDS : CRABML_HIP_TAP_PLAN_WORDS;
  const char* const hook;  // the entry point's name, for its error texts
  int layer = -1;          // the armed layer, -1 = disarmed
  char* buf = nullptr;     // the scratch area (device), in the device's own layouts; every field 256-aligned
  size_t cap = 0, used = 0;
  size_t off[FIELDS] = {}, len[FIELDS] = {};
  int32_t plan[WORDS] = {};
  // a fresh directory and plan, then armed (the overflow recomputation of a prompt chunk arms again: it starts afresh)
  void arm(int l) {
    used = 0;
    for (int f = 0; f < FIELDS; f++) off[f] = len[f] = 0;
    for (auto& v : plan) v = 0;
    layer = l;
  }
  void disarm() { layer = -1; }
  bool armed() const { return layer >= 0; }
  void note(int word, int32_t value) {
    if (armed()) plan[word] = value;
  }
  void note(int l, int word, int32_t value) {  // a decision of layer l
    if (layer == l) plan[word] = value;
  }
  int ensure(crabml_hip_llama* c, size_t bytes);
  int copy(crabml_hip_llama* c, int f, const void* src, size_t bytes);
  int read_back(crabml_hip_device* dev, std::vector<uint8_t>* host) const;
};
// what a hook's entry point says of a field: raw bytes (f32 values, f16 planes; cols = 0) or `rows` rows of `cols` elements as `qtype` planes
struct TapField {
  uint32_t qtype = CRABML_HIP_F32;
  size_t cols = 0, rows = 1;
  int qp_of = -1;  // >= 0: no copy of its own -- the class-major plane (cols bytes per row) inside the Q8_K planes field `qp_of` copied
};

// What a context runs, as one value: decide_step makes it at create, every reader goes through c->plan, and
// crabml_hip_debug_step_plan (crabml_hip_debug.h) hands it out.
enum class SegPath { PerOp = 0, Fused5 = 1, FusedK = 2 };  // enqueue_segment_generic / enqueue_segment_t / enqueue_segment_k
struct StepPlan {
  SegPath path = SegPath::PerOp;
  bool ordered = false;        // strict-order device: the fused launches with block-ordered sums (Fused5: k_*_ord; FusedK: the ORD forms)
  // ---- the segment forms
  bool norm_epi = false;       // Fused5: RMSNorm + quantize run in the wo / ffn_down epilogue (tp > 1: over a P2P group or in the dry run,
                               // where the epilogue hosts the collective too)
  bool norm_epi_k = false;     // the same for a K-quant body's layers (Q8_K planes out of the epilogue)
  // the hop-free norm of the fast step (Q4_0 / Q8_0 layers, one GPU): wo quantizes x * w_norm block by block and leaves 1 / rms to
  // the gate/up launch (RmsTail, gemv_core.hpp) -- no in-launch gather.  Off: CRABML_HIP_LLAMA_EXACT_NORM, strict order, tp.
  bool defer_norm = false;
  int gu_rows = 0;             // > 0 (tensor-parallel ranks): gate/up leaves h as f32 from workgroups of this many rows, ffn_down quantizes it
  bool q8k_producers = false;  // attention / gate-up emit the Q8_K planes of wo's / ffn_down's rhs themselves
  bool k_norm_in = false;      // fast Q4_K step: gate | up normalizes and quantizes wo's f32 row itself (k_gateup_k_lds<.., NORMIN>)
  // ---- the attention forms (attn_variant 0 = one workgroup per head, 1 = the long-context kernels, 2 = variant 1's ticket form)
  bool attn_long_ok = false;   // variant 1 exists: exact_long_ok or attn_flash
  bool exact_long_ok = false;  // the exact long-context kernels (score / probability rows of seq_len elements read as 16-byte vectors):
                               // f16 cache, head_dim % 32 == 0, group size in {1, 2, 4, 8}, seq_len % 8 == 0
  size_t attn_long_from = 0;   // cached positions (pos + 1) from which variant 1 is used
  bool pv_split = false;       // variant 1, exact: k_attn_pv_split (products by producer waves) instead of k_attn_pv
  bool attn_flash = false;     // variant 1 of the FAST step: k_attn_flash (split-KV, f32 accumulation) instead of the three exact kernels
  bool flash_ticket = false;   // A/B: the merge by the last-arriving workgroup inside k_attn_flash instead of its own launch
  size_t flash_ticket_until = 0;  // > 0: positions [attn_long_from, this) run variant 2
  bool attn_flash_rows = false;   // the batched prefill's attention runs k_attn_flash_rows (fast step, f16 cache, head_dim 64 / 128)
  int flash_S = 0;                // position slices (workgroups) per kv head
  int flash_min_rows = FLASH_MIN_ROWS;  // cached rows per active slice, at least
  int attn_s_rows = 0;         // > 0: variant 0 runs k_attn_s (K / V staged through LDS) with room for this many cached rows
  size_t attn_s_lds = 0;
};

struct crabml_hip_llama {
  crabml_hip_device* dev = nullptr;
  crabml_hip_llama_config_t cfg{};
  uint32_t wtype = 0;
  StepPlan plan;  // which launches the context runs (decide_step)
  int tp = 1, tp_rank = 0;
  crabml_hip_tp_comm* comm = nullptr;
  // local (per-rank) geometry
  int hd = 0, npairs = 0, n_heads_l = 0, n_kv_l = 0, dim_l = 0, kv_dim_l = 0, hidden_l = 0;
  std::vector<crabml_hip_buf*> held;  // retained weight buffers
  crabml_hip_buf* token_embed = nullptr;
  crabml_hip_buf* rms_final = nullptr;
  crabml_hip_buf* output = nullptr;
  std::vector<crabml_hip_buf*> rms_att, rms_ffn, wq, wk, wv, wo, gate, down, up;
  // Qwen2 (crabml_hip_llama_create_arch): q / k / v biases per layer, NEOX rope (the q|k|v kernels' QKV_QWEN2 form)
  bool qwen2 = false;
  std::vector<crabml_hip_buf*> bq, bk, bv;
  // Gemma (llama2.rs:455-524): the embedded row times sqrtf(dim), NEOX rope without biases (QKV_GEMMA), h = gelu(g) * u
  bool gemma = false;
  float embed_scale = 1.0f;    // k_embed's factor: 1.0f = none
  FfnAct ffn_act{nullptr, 0};  // what every gate | up launch of this context is handed: SiLU + the exp table, or GELU + the gelu table
  // device state
  std::vector<void*> kc, vc;
  size_t kv_bytes = 0;
  float* x = nullptr;        // residual stream (dim), replicated on every rank
  float* partial = nullptr;  // tp > 1: this rank's wo / ffn_down partial sums (dim), all-reduced in place
  float* qbuf = nullptr;     // roped, scaled q (dim_l)
  float* attn = nullptr;     // attention output (dim_l)
  float* h = nullptr;        // ffn hidden as f32 (hidden_l): the per-op and K-quant segments, and ffn_down's prologue under gu_rows
  float* logits = nullptr;   // vocab
  float* host_logits = nullptr; // lazy.hip: pinned host copy of the logits, written by a kernel behind the classifier; the two words
                                // behind the vocab_size floats are {sequence number of the step that wrote them, its fault word}
  unsigned out_seq = 0;         // sequence number of the last step whose logits were sent to host_logits
  unsigned lazy_serial = 0;     // lazy.hip: the step serial is set by the host at every begin (see lazy_ctx_begin)
  bool ext_kv = false;          // lazy.hip: kc / vc are the runner's own cache buffers (retained in `held`), not allocations of ours
  const crabml_hip_buf* ext_kc0 = nullptr;  // ... the first layer's K cache handle (lazy_ctx_orphaned)
  float* tmp = nullptr;      // per-op segments: the GEMV outputs (q | k | v, gate | up, wo / ffn_down in front of the residual add)
  char* act_dim = nullptr;   // planes of the normalized residual (dim) in the rhs type `qt` (the final row: `out_qt`)
  char* act_attn = nullptr;  // `qt` planes of the attention output (dim_l)
  char* act_hid = nullptr;   // `qt` planes of the ffn hidden vector (hidden_l)
  float* rope = nullptr;     // [seq_len][npairs][2]
  int* state = nullptr;      // token, pos, step, sink, serial (never reset), fault
  unsigned long long* slots = nullptr;  // dim/32 {chunk sum, epoch} granules of the norm epilogue
  unsigned long long* a8gran = nullptr;  // Q4_K layers: granules of the attention output (dim_l) and of h (hidden_l), through which
  unsigned long long* h8gran = nullptr;  // the producing kernels assemble Q8_K super-blocks (q8k_exchange_store)
  unsigned tp_salt = 0;      // P2P group: epoch salt of this context (see TpP2P::salt)
  bool tp_dry = false;       // CRABML_HIP_LLAMA_TP_DRY_RUN: a lone rank that skips the all-reduces (timing only)
  uint32_t qt = 0, out_qt = 0;  // vec_dot_rhs_dtype of the layer weights / of the classifier
  float* xn = nullptr;       // generic path: normalized residual (f32, dim)
  float* rsums = nullptr;    // [dim / 16] chunk sums of squares of the residual stream
  unsigned* out_tokens = nullptr;
  int out_cap = 0;
  float* am_val = nullptr;  // argmax partials
  int* am_idx = nullptr;
  // CRABML_HIP_LLAMA_TP_SPLIT_VOCAB: this rank's classifier rows [vocab_off, vocab_off + vocab_l) (otherwise 0 / vocab_size)
  bool split_vocab = false;
  int vocab_l = 0, vocab_off = 0;
  int* am_best = nullptr;   // {max bits, index} of this rank's shard (single-device simulation: combined by the driver)
  // temperature / top-p sampler (crabml_hip_llama_decode_sample), allocated on first use: block maxima, the keys of the
  // vocabulary, the key histogram (zero between steps), {temperature, topp}, one coin per step
  bool sampling = false;     // the final segment ends in the sampler instead of the arg-max (enqueue_classifier_and_sampler)
  float* sm_bmax = nullptr;
  unsigned short* sm_keys = nullptr;
  unsigned* sm_hist = nullptr;
  float* sm_par = nullptr;
  float* sm_coins = nullptr;
  hipGraph_t sgraph[3] = {nullptr, nullptr, nullptr};  // the step with the sampler, per attention variant, captured on first use
  hipGraphExec_t sexec[3] = {nullptr, nullptr, nullptr};
  size_t kv_len = 0;
  // [0]: one attention workgroup per head; [1]: the long-context attention kernels (from attn_long_from positions)
  hipGraph_t graph[3] = {nullptr, nullptr, nullptr};
  hipGraphExec_t exec[3] = {nullptr, nullptr, nullptr};
  bool use_graph = false;
  bool capturing = false;
  int attn_variant = 0;         // which of them the next enqueue emits: 0 = one workgroup per head, 1 = the long-context kernels,
                                // 2 = split-KV attention with the merge inside the launch (ticket form: the mid range)
  float* flash_part = nullptr;  // [n_kv_l][flash_S][G][hd + 2] partial {O, m, l}
  unsigned* flash_tick = nullptr;  // [n_kv_l] arrival counters (monotonic)
  float* scores_g = nullptr;    // [n_heads_l][seq_len] f32
  unsigned short* p16 = nullptr;  // [n_heads_l][seq_len] f16 probabilities
  // batched prefill (crabml_hip_llama_prefill): row buffers for pf_cap prompt rows, allocated on first use
  size_t pf_cap = 0;
  int* pf_tokens = nullptr;
  float *pf_x = nullptr, *pf_xn = nullptr, *pf_q = nullptr, *pf_k = nullptr, *pf_v = nullptr, *pf_qr = nullptr, *pf_attn = nullptr,
        *pf_tmp = nullptr, *pf_g = nullptr, *pf_u = nullptr;
  char *pf_act_dim = nullptr, *pf_act_hid = nullptr;
  float* pf_split = nullptr;  // ... and pf_split_floats of scratch for the partial tiles of its k pieces
  size_t pf_split_floats = 0;
  int* pf_ovf = nullptr;   // raised by the writers of pf_xh / pf_xh2 when a B' value is +-inf (prefill_chunk recomputes the chunk)
  void* pf_xh2 = nullptr;  // a second one: the gate | up launch reads pf_xh while its epilogue writes ffn_down's
  void* pf_xh = nullptr;  // the fast pass's f16 GEMMs: the current rhs rows as pre-scaled f16 (gemm_f16w.hip), gemm_f16w_xh_bytes(cap, max(dim, hidden))
  float* pf_scores = nullptr;          // long prompts: [PF_LONG_ROWS][n_heads][seq_len] f32 scores
  unsigned short* pf_p16 = nullptr;    //               and f16 probabilities, allocated on first use
  std::vector<std::pair<void*, size_t>> allocs;
  // token / pos / step of the next step are staged in pinned host memory owned by the context (a ring, one slot per
  // set_state): the async copy reads it when the stream gets there, long after the caller's stack frame is gone
  int* h_state = nullptr;
  unsigned h_state_next = 0;
  static constexpr unsigned H_STATE_SLOTS = 256;
  // the two parity taps (test hooks, crabml_hip_debug.h): crabml_hip_llama_debug_tap arms `tap` for one eager decode step
  // (enqueue_segment_t / enqueue_segment_k), crabml_hip_llama_debug_prefill_tap arms `pftap` for one chunk pass of the prompt path (prefill_chunk_pass,
  // where every field holds all rows of the pass); a scratch area each, allocated on the hook's first call
  TapRec tap{"llama debug_tap"}, pftap{"llama debug_prefill_tap"};
};

// ---- lazy.hip's context: token / position / serial of a step straight from kernel arguments (a launch on the stream's own queue:
// no copy-engine hand-off in front of the step's first kernel), and the logits to pinned host memory by a kernel behind the
// classifier, followed by a flag the host can spin on (no copy-engine hand-off, no interrupt-driven wait behind the step's last)
__global__ void k_set_state5(int* __restrict__ st, int token, int pos, int step, int serial, int out_seq) {
  st[0] = token;
  st[1] = pos;
  st[2] = step;
  st[4] = serial;
  st[7] = out_seq;  // what k_host_flag raises when this step's logits have reached the host
}
__global__ __launch_bounds__(256) void k_logits_to_host(const f32x4* __restrict__ src, f32x4* __restrict__ dst, int n4, const float* __restrict__ src1,
                                                        float* __restrict__ dst1, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) __builtin_nontemporal_store(src[i], dst + i);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst1[n4 * 4 + threadIdx.x] = src1[n4 * 4 + threadIdx.x];
}
__global__ void k_host_flag(unsigned* __restrict__ flag, const int* __restrict__ seq_d, const int* __restrict__ fault) {
  const unsigned seq = (unsigned)*seq_d;  // (from device memory: the launch may be a node of the step's replayed graph)
  flag[1] = (unsigned)*fault;
  __threadfence_system();  // (the copy kernel has completed: stream order; this orders the fault word before the flag)
  __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

namespace {

TpP2P p2p_view(const crabml_hip_tp_comm* m);
// the inbox view a decode-step kernel gets: empty (n = 0) unless this context runs the fused collective; timeouts raise the
// context's own fault word, which forward / decode_greedy check at their sync
TpP2P tp_view(const crabml_hip_llama* c, bool fused_collective) {
  TpP2P t = p2p_view(fused_collective && c->comm && c->comm->p2p ? c->comm : nullptr);  // dry run: no comm, n = 0
  t.fault = c->state + 5;
  t.salt = c->tp_salt;
  return t;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the kernel in this PROCESS, not of a context: a second context
// with a shorter sequence must not lower the limit an earlier context's launches (and captured graphs) were sized for.
// Only ever raise it, per device.
hipError_t raise_dyn_lds(const crabml_hip_device* dev, const void* fn, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> have;
  if (dev->dry) return hipErrorNoDevice;  // record-only test device
  std::lock_guard<std::mutex> g(mu);
  int& cur = have[{dev->ordinal, fn}];
  if (bytes <= cur) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) cur = bytes;
  return e;
}

// k_attn (one workgroup per head): a score row of `row` positions and q, f32, in the dynamic LDS a launch gets without asking
constexpr size_t K_ATTN_LDS = 64 * 1024;
constexpr size_t k_attn_lds_bytes(size_t row, size_t hd) { return (row + hd) * sizeof(float); }

int dalloc(crabml_hip_llama* c, size_t bytes, void** out) {
  size_t cap = 0;
  CH_TRY(pool_alloc(c->dev, bytes, out, &cap));
  c->allocs.push_back({*out, cap});
  return 0;
}

Planes planes_of(const crabml_hip_buf* b) {
  return Planes{(const i32x4*)b->ptr, scale_plane<unsigned short>(b)};
}

// the planes of a 32-block activation (Q8_0: q | d | isum i32;  Q8_1: q | d | s f16) as the kernels write them
struct ActPtrs {
  signed char* q;
  unsigned short* d;
  void* isum;  // the format's third plane
};
ActPtrs act_ptrs(char* p, size_t n, uint32_t qt) {
  ActLayout al = act_layout(qt, n);
  return ActPtrs{(signed char*)p, (unsigned short*)(p + al.off_d), (void*)(p + al.off_aux)};
}
// the same planes as the view a kernel reads: act_at over the offsets act_ptrs applied
template <int FMT>
typename ActOf<FMT>::type act_view(const ActPtrs& a) {
  ActLayout al;
  al.off_d = (size_t)((const char*)a.d - (const char*)a.q);
  al.off_aux = (size_t)((const char*)a.isum - (const char*)a.q);
  return act_at<typename ActOf<FMT>::type>((const char*)a.q, al);
}

int n_segments(const crabml_hip_llama* c) { return 2 * (int)c->cfg.n_layers + 1; }

// Workgroups per 32-row chunk of a wo / ffn_down launch whose rows are k elements long: two for long rows (ffn_down), so that every
// CU streams (a CU sustains ~26 GB/s here) -- while the dim / 32 chunks still fit the chip twice.  x_only (the fast Q4_K wo that
// leaves x alone, k_norm_in): no hop pairs the halves of a chunk, so two 16-row workgroups per chunk whenever that fits.
// The one place that decides it: the launches, the LDS checks of llama_create_impl and gate | up's sum_parts all ask here
// (the plan words CRABML_HIP_PLAN_SPLIT_WO / _DOWN of crabml_hip_debug.h record it, under its former name split_of).
int chunk_split(uint64_t flags, int k, int dim, int n_cu, bool x_only = false) {
  return (flags & CRABML_HIP_LLAMA_SPLIT_CHUNKS_ALWAYS)  ? 2
         : (flags & CRABML_HIP_LLAMA_SPLIT_CHUNKS_NEVER) ? 1
         : (k / 32 >= 256 && dim / 32 <= n_cu)           ? 2
         : (x_only && dim / 32 <= n_cu)                  ? 2
                                                         : 1;
}

// Whether a wo / ffn_down launch (k_gemv_res_nq over a 32-element format, its rhs planes in global memory) copies those planes into
// LDS once per workgroup and requests a row's weights NQ_DEEP steps ahead (rows_partial_deep): the depth, or 0 = every wave reads its
// units from global memory, two per request round -- the loop every such launch had.  Inputs: the row's length, the rows per
// wave, the resident waves per CU.  Measured (profiles/request_rounds.md): with one row per wave and one 1024-thread workgroup per CU
// (ffn_down: two workgroups per chunk, 16 waves on a CU and nothing else to cover their waits) the copy pays, 8.55 -> 7.97 us on the
// 8B shape.  Two rows per wave (one workgroup per chunk: wo) keep the old loop: at k = 4096 in Q4_0 that is the whole row in one
// round already, and its blocks of 4 steps x 2 rows do not fit the workgroup's 128 VGPRs.  No threshold on the steps: chunk_split
// gives two workgroups per chunk from 256 blocks on, four steps and more; shorter rows come here under SPLIT_CHUNKS_ALWAYS alone.
// k <= ACT_STAGE_MAX_K: what the copy's two pieces per thread cover.  The one place that decides it;
// A/B: CRABML_HIP_LLAMA_NQ_TWO_UNIT_ROUNDS.
int nq_request_depth(uint64_t flags, int k, int rows_per_wave, int waves_per_cu) {
  if ((flags & CRABML_HIP_LLAMA_NQ_TWO_UNIT_ROUNDS) || rows_per_wave != 1 || waves_per_cu > 16 || k > ACT_STAGE_MAX_K) return 0;
  return NQ_DEEP;
}

// The norm kernels walk a row with 1024 threads x NIT float4 iterations: rows past 4096 elements take 12 (llama_create_impl stops at
// 12288).  The one place that knows; CRABML_HIP_PLAN_NORM_NIT records this value.
int norm_nit(int dim) { return dim <= 4096 ? 4 : 12; }
void launch_norm_f32(hipStream_t st, float* x, const float* addv, const float* wn, int dim, float eps, float* out, int half) {
  with_const_else<4, 12>(norm_nit(dim), [&](auto nit) {
    k_norm_f32<decltype(nit)::value><<<1, 1024, norm_lds_bytes(dim), st>>>(x, addv, wn, dim, eps, out, half);
  });
}

// The kernels whose dynamic-LDS limit llama_create_impl raises: create and the launch site take the function pointer from the same
// selector (as flash_kernel below), so the instantiation that was raised is the one that runs.
typedef decltype(&k_attn_pv_split<1>) PvSplitFn;
struct PvSplitKernel {
  PvSplitFn fn = nullptr;
  int nsub = 0, threads = 0;
  size_t lds = 0;
};
// (two heads per workgroup from group 2 on: an odd group has no such kernel and keeps k_attn_pv, which is bit-identical)
PvSplitKernel pv_split_kernel(int grp) {
  PvSplitKernel k;
  with_const<1, 2, 4, 6, 8>(grp, [&](auto g) {
    typedef PvSplit<decltype(g)::value> P;
    k = PvSplitKernel{k_attn_pv_split<decltype(g)::value>, P::NSUB, P::THREADS, P::LDS};
  });
  return k;
}
typedef decltype(&k_attn_s<0>) AttnSFn;
AttnSFn attn_s_kernel(int hd) { return hd == 128 ? k_attn_s<128> : k_attn_s<0>; }
typedef decltype(&k_attn_flash_rows<64>) FlashRowsFn;
FlashRowsFn flash_rows_kernel(int hd) { return hd == 128 ? k_attn_flash_rows<128> : hd == 64 ? k_attn_flash_rows<64> : nullptr; }
// strict-order Q4_K step: k_gemv_res_nq<Q4_K, SPLIT, QIN, .., ORD> (qin 1 = quantize the f32 rhs, 2 = copy finished planes) ...
typedef decltype(&k_gemv_res_nq<CRABML_HIP_Q4_K, 1, 1, false, false, true>) NqOrdKFn;
NqOrdKFn nq_ord_k_kernel(int split, int qin) {
  NqOrdKFn fn = nullptr;
  with_const_else<2, 1>(split, [&](auto s) {
    with_const_else<2, 1>(qin, [&](auto q) { fn = k_gemv_res_nq<CRABML_HIP_Q4_K, decltype(s)::value, decltype(q)::value, false, false, true>; });
  });
  return fn;
}
// ---- the K-quant bodies of the fused step: THE list ----------------------------------------------------------------------------
// A format named here has its launches instantiated, dispatched (enqueue_segment, gateup_k_kernel, gemv_out), admitted with its mixes
// (validate_weights) and routed (decide_step).  Everything a row says comes from the format's device policy (KBody, gemv_core.hpp).
typedef FmtList<CRABML_HIP_Q4_K, CRABML_HIP_Q5_K, CRABML_HIP_Q6_K, CRABML_HIP_Q3_K, CRABML_HIP_Q2_K> KBodies;
struct KBodyRow {
  int fmt;
  bool epi_only;  // built in the norm-epilogue form only
  bool v_whole;   // an alternate comes as its whole buffer, attn_v and ffn_down only; else attn_v, attn_output and ffn_down by their own format
  int n_alt;
  int alt[2];     // VAlt: the formats those tensors may have beside fmt
  bool takes(uint32_t t) const {
    for (int i = 0; i < n_alt; i++)
      if ((uint32_t)alt[i] == t) return true;
    return false;
  }
};
template <int FMT, int... ALT>
constexpr KBodyRow k_body_row(FmtList<ALT...>) {
  return KBodyRow{FMT, KBody<FMT>::EPI_ONLY, KBody<FMT>::V_WHOLE, (int)sizeof...(ALT), {ALT...}};
}
template <int... FMTS>
const KBodyRow* k_body_of(FmtList<FMTS...>, uint32_t t) {
  static constexpr KBodyRow rows[] = {k_body_row<FMTS>(typename KBody<FMTS>::VAlt{})...};
  for (const KBodyRow& r : rows)
    if ((uint32_t)r.fmt == t) return &r;
  return nullptr;
}
// the row of format t, nullptr when t is no K-quant body
const KBodyRow* k_body_of(uint32_t t) { return k_body_of(KBodies{}, t); }
// f(integral_constant<format>) for the format of the list that v names; false when it names none
template <int... FMTS, class F>
bool with_fmt(FmtList<FMTS...>, int v, F&& f) {
  return with_const<FMTS...>(v, f);
}
// ... and for a tensor of a BODY's layer that is launched by its own format: one of the body's alternates, else the body's
template <int BODY, int... ALT, class F>
void with_body_or_alt(FmtList<ALT...>, int v, F&& f) {
  with_const_else<ALT..., BODY>(v, f);
}

// ... and the forms of k_gateup_k_lds<QOUT, ORD, NORMIN, BODY> that exist (NORMIN writes planes and has no ordered form; nor has a body
// other than Q4_K)
typedef decltype(&k_gateup_k_lds<false>) GateupKFn;
GateupKFn gateup_k_kernel(bool qout, bool ord, bool normin, int body = CRABML_HIP_Q4_K) {
  if (ord) return qout ? k_gateup_k_lds<true, true> : k_gateup_k_lds<false, true>;
  GateupKFn fn = nullptr;
  with_fmt(KBodies{}, body, [&](auto b) {
    constexpr int BODY = decltype(b)::value;
    fn = normin ? k_gateup_k_lds<true, false, true, BODY> : qout ? k_gateup_k_lds<true, false, false, BODY> : k_gateup_k_lds<false, false, false, BODY>;
  });
  return fn;
}

}  // namespace

// (a shorter area of an earlier call stays with the context until it is destroyed)
int TapRec::ensure(crabml_hip_llama* c, size_t bytes) {
  if (cap >= bytes) return 0;
  cap = 0;
  CH_TRY(dalloc(c, bytes, (void**)&buf));
  cap = bytes;
  return 0;
}
// field `f` = `bytes` bytes at `src` as the stream finds them here
int TapRec::copy(crabml_hip_llama* c, int f, const void* src, size_t bytes) {
  if (!armed() || src == nullptr || bytes == 0) return 0;
  if (c->capturing) CH_BAIL(c->dev, CRABML_HIP_UNEXPECTED, "%s: a tapped step is never captured", hook);
  if (f < 0 || f >= FIELDS) CH_BAIL(c->dev, CRABML_HIP_UNEXPECTED, "%s: no field %d", hook, f);
  // a field copied a second time with the same length (the prompt pass's one-launch GEMM declined after its B' was tapped: the separate
  // launches tap it again) takes its slot again -- the area holds every field once
  const bool again = len[f] == bytes;
  const size_t at = again ? off[f] : align_up(used, 256);
  if (at + bytes > cap) CH_BAIL(c->dev, CRABML_HIP_UNEXPECTED, "%s: scratch area too small", hook);
  CH_HIP(c->dev, hipMemcpyAsync(buf + at, src, bytes, hipMemcpyDeviceToDevice, c->dev->stream));
  if (again) return 0;
  off[f] = at;
  len[f] = bytes;
  used = at + bytes;
  return 0;
}
// the used part of the scratch area to `host`, in stream order (the caller synchronizes)
int TapRec::read_back(crabml_hip_device* dev, std::vector<uint8_t>* host) const {
  host->resize(used ? used : 1);
  if (used) CH_HIP(dev, hipMemcpyAsync(host->data(), buf, used, hipMemcpyDeviceToHost, dev->stream));
  return 0;
}

namespace {

// What the host receives of a tap: field after field (8-aligned) in `dst` with its place in `dir`, raw fields as they are, planes
// re-packed as the reference's blocks (never larger than the planes), and the first `nwords` plan words as field `plan_field`.
// `host` = the scratch area as read_back left it.
int export_fields(crabml_hip_device* dev, const TapRec& t, const std::vector<uint8_t>& host, const TapField* fld, int nfields, int plan_field,
                  int nwords, void* dst, size_t dst_bytes, crabml_hip_tap_entry_t* dir) {
  uint8_t* o = (uint8_t*)dst;
  size_t at = 0;
  for (int f = 0; f < nfields; f++) {
    dir[f] = crabml_hip_tap_entry_t{at, 0, fld[f].qtype, 0};
    const uint8_t* src = host.data() + t.off[f];
    size_t out_bytes = t.len[f];
    if (f == plan_field) {  // host words, not a device buffer
      src = (const uint8_t*)t.plan;
      out_bytes = (size_t)nwords * sizeof(int32_t);
    }
    if (fld[f].qp_of >= 0) {  // rows of Q8_K planes -> their class-major planes, as the device holds them
      const int pf = fld[f].qp_of;
      const ActLayout al = act_layout(CRABML_HIP_Q8_K, fld[f].cols);
      out_bytes = fld[f].rows * fld[f].cols;
      if (t.len[pf] == 0) continue;
      if (t.len[pf] != fld[f].rows * al.total || at + out_bytes > dst_bytes)
        CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "%s: field %d has an unexpected size", t.hook, f);
      for (size_t r = 0; r < fld[f].rows; r++) memcpy(o + at + r * fld[f].cols, host.data() + t.off[pf] + r * al.total + al.off_p, fld[f].cols);
      dir[f].bytes = out_bytes;
      at += align_up(out_bytes, 8);
      continue;
    }
    if (out_bytes == 0) continue;
    if (fld[f].cols == 0) {
      if (at + out_bytes > dst_bytes) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "%s: field %d does not fit dst", t.hook, f);
      memcpy(o + at, src, out_bytes);
    } else {  // rows of planes -> rows of blocks
      const uint32_t qt = fld[f].qtype;
      const size_t row_planes = act_layout(qt, fld[f].cols).total, row_blocks = fld[f].cols / block_elems(qt) * block_bytes(qt);
      out_bytes = fld[f].rows * row_blocks;
      if (t.len[f] != fld[f].rows * row_planes || at + out_bytes > dst_bytes)
        CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "%s: field %d has an unexpected size", t.hook, f);
      for (size_t r = 0; r < fld[f].rows; r++) planes_to_blocks(qt, fld[f].cols, src + r * row_planes, o + at + r * row_blocks);
    }
    dir[f].bytes = out_bytes;
    at += align_up(out_bytes, 8);
  }
  return 0;
}

// attention of layer l (llama2.rs:571-590): qbuf x KV cache -> attn (f32), plus its Q8_0 planes for wo when xq != NULL.
// Emits the variant selected in c->attn_variant (0: one workgroup per head, 1: the long-context kernels).
template <int G>
void launch_attn_long(crabml_hip_llama* c, int l, signed char* xq, unsigned short* xd, void* xisum, bool prof) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const int hd = c->hd, seq_cap = (int)c->cfg.seq_len, n_kv = c->n_kv_l;
  const int* pos_d = c->state + 1;
  const int ts = 256 / G, nsplit = (seq_cap + ts - 1) / ts;
  crabml_hip_device::ProfRec r[3];
  for (int i = 0; i < 3; i++)
    if (prof) prof_begin(dev, &r[i], CRABML_HIP_F32, 7 + i, 0.0);  // stages 7 / 8 / 9: scores / softmax / pv
  launch_k(st, prof ? &r[0] : nullptr, k_attn_scores<G>, dim3(n_kv * nsplit), dim3(256), (size_t)G * hd * sizeof(float),
           (const float*)c->qbuf, (const unsigned short*)c->kc[l], pos_d, c->scores_g, n_kv, hd, seq_cap, nsplit, 0);
  launch_k(st, prof ? &r[1] : nullptr, k_attn_softmax<16>, dim3(c->n_heads_l), dim3(1024), (size_t)seq_cap * sizeof(float),
           (const float*)c->scores_g, pos_d, (const unsigned short*)dev->exp_table, c->p16, seq_cap, 0, dev->strict_order ? 1 : 0);
  if (c->plan.pv_split) {
    const PvSplitKernel pv = pv_split_kernel(G);
    launch_k(st, prof ? &r[2] : nullptr, pv.fn, dim3(n_kv * (hd / 32) * pv.nsub), dim3(pv.threads), pv.lds,
             (const unsigned short*)c->p16, (const unsigned short*)c->vc[l], pos_d, c->attn, xq, xd, xisum, hd, seq_cap,
             c->qt == CRABML_HIP_Q8_1 ? 1 : 0, 0);
  } else
    launch_k(st, prof ? &r[2] : nullptr, k_attn_pv<G>, dim3(n_kv * (hd / 32)), dim3(256), 0, (const unsigned short*)c->p16,
             (const unsigned short*)c->vc[l], pos_d, c->attn, xq, xd, xisum, hd, seq_cap, c->qt == CRABML_HIP_Q8_1 ? 1 : 0, 0);
  for (int i = 0; i < 3; i++)
    if (prof) prof_end(dev, &r[i]);
}

// the k_attn_flash instantiation for (G, hd, rhs type of wo); nullptr = no such kernel
typedef void (*FlashFn)(const float*, const unsigned short*, const unsigned short*, const int*, float*, unsigned*, float*, signed char*,
                        unsigned short*, void*, int, int, int);
template <int G, int HD>
FlashFn flash_kernel_gh(bool q81, bool ticket) {
  if (ticket) return q81 ? (FlashFn)k_attn_flash<G, HD, true, true> : (FlashFn)k_attn_flash<G, HD, false, true>;
  return (FlashFn)k_attn_flash<G, HD, false, false>;
}
// (groups 3, 5, 6 and 7 -- Llama-3.2-3B; Qwen2.5-14B / 32B; 1.5B; 7B / 0.5B -- exist at head_dim 64 and 128 only: no model served has one
// of them at 256)
template <int G>
FlashFn flash_kernel_g(int hd, bool q81, bool ticket) {
  if constexpr (G == 1 || G == 2 || G == 4 || G == 8) {
    if (hd == 256) return flash_kernel_gh<G, 256>(q81, ticket);
  }
  if (hd == 128) return flash_kernel_gh<G, 128>(q81, ticket);
  if (hd == 64) return flash_kernel_gh<G, 64>(q81, ticket);
  return nullptr;
}
FlashFn flash_kernel(int grp, int hd, bool q81, bool ticket) {
  FlashFn fn = nullptr;
  with_const<1, 2, 3, 4, 5, 6, 7, 8>(grp, [&](auto g) { fn = flash_kernel_g<decltype(g)::value>(hd, q81, ticket); });
  return fn;
}
// which attention form serves cache position `pos` (see attn_variant)
int variant_of(const crabml_hip_llama* c, size_t pos) {
  if (!(c->plan.attn_long_ok && pos + 1 >= c->plan.attn_long_from)) return 0;
  return c->plan.flash_ticket_until > 0 && pos + 1 < c->plan.flash_ticket_until ? 2 : 1;
}
void launch_attn_flash(crabml_hip_llama* c, int l, signed char* xq, unsigned short* xd, void* xisum, bool prof) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const int hd = c->hd, grp = c->n_heads_l / c->n_kv_l;
  const bool q81 = c->qt == CRABML_HIP_Q8_1;
  const bool ticket = c->plan.flash_ticket || c->attn_variant == 2;
  const FlashFn fn = flash_kernel(grp, hd, q81, ticket);
  crabml_hip_device::ProfRec r[2];
  if (prof) prof_begin(dev, &r[0], CRABML_HIP_F32, 7, 0.0);
  launch_k(st, prof ? &r[0] : nullptr, fn, dim3(c->n_kv_l * c->plan.flash_S), dim3(flash_threads(grp)), flash_lds_bytes(grp, hd),
           (const float*)c->qbuf, (const unsigned short*)c->kc[l], (const unsigned short*)c->vc[l], (const int*)(c->state + 1), c->flash_part,
           c->flash_tick, c->attn, xq, xd, xisum, (int)c->cfg.seq_len, c->plan.flash_S, c->plan.flash_min_rows);
  if (prof) prof_end(dev, &r[0]);
  if (ticket) return;
  if (prof) prof_begin(dev, &r[1], CRABML_HIP_F32, 8, 0.0);
  crabml_hip_device::ProfRec* R1 = prof ? &r[1] : nullptr;
  const int* pos_d = c->state + 1;
  with_const_else<256, 128, 64>(hd, [&](auto hdc) {  // (flash_kernel has no other head_dim)
    with_const_else<0, 1>(q81, [&](auto q) {
      constexpr int HD = decltype(hdc)::value;
      launch_k(st, R1, k_attn_flash_merge<HD, decltype(q)::value != 0>, dim3(c->n_heads_l), dim3(HD), 0, (const float*)c->flash_part, pos_d,
               c->attn, xq, xd, xisum, grp, c->plan.flash_S, c->plan.flash_min_rows);
    });
  });
  if (prof) prof_end(dev, &r[1]);
}

int enqueue_attention(crabml_hip_llama* c, int l, signed char* xq, unsigned short* xd, void* xisum, const PrefetchPlan& pf,
                      int spare, bool prof, const AttnQ8K* k8 = nullptr) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const int hd = c->hd, seq_cap = (int)c->cfg.seq_len, n_heads = c->n_heads_l, n_kv = c->n_kv_l;
  const int* pos_d = c->state + 1;
  if (c->attn_variant >= 1 && c->plan.attn_flash) {
    launch_attn_flash(c, l, xq, xd, xisum, prof);
    return 0;
  }
  if (c->attn_variant >= 1) {  // (attn_long_ok: the group size is one of these)
    with_const_else<1, 2, 3, 4, 5, 6, 7, 8>(n_heads / n_kv, [&](auto grp) { launch_attn_long<decltype(grp)::value>(c, l, xq, xd, xisum, prof); });
    return 0;
  }
  // (k_attn's score row spans the cache here: create admits a cache past K_ATTN_LDS only where k_attn_s serves this variant)
  const size_t attn_lds = k_attn_lds_bytes(seq_cap, hd);
  if (c->plan.attn_s_rows == 0 && attn_lds > K_ATTN_LDS)
    CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: decode attention would need a score row of %d positions in LDS", seq_cap);
  const int sbit = dev->strict_order ? 256 : 0;  // strict device: sequential softmax row sums at any length (softmax.rs:43-48)
  crabml_hip_device::ProfRec ar{};
  crabml_hip_device::ProfRec* AR = prof ? &ar : nullptr;
  if (prof) prof_begin(dev, &ar, CRABML_HIP_F32, 7, 0.0);
  if (c->plan.attn_s_rows > 0)
    launch_k(st, AR, attn_s_kernel(hd), dim3(n_heads + spare), dim3(256), c->plan.attn_s_lds, (const float*)c->qbuf, (const unsigned short*)c->kc[l],
             (const unsigned short*)c->vc[l], pos_d, (const unsigned short*)dev->exp_table, c->attn, xq, xd, xisum, n_heads, n_kv, hd, seq_cap,
             c->plan.attn_s_rows, pf, (k8 ? 2 : c->qt == CRABML_HIP_Q8_1 ? 1 : 0) | sbit, (long long*)nullptr, k8 ? *k8 : AttnQ8K{});
  else
    with_const_else<0, 1>(c->cfg.use_f16_kv_cache != 0, [&](auto kv16) {
      launch_k(st, AR, k_attn<decltype(kv16)::value != 0>, dim3(n_heads + spare), dim3(256), attn_lds, (const float*)c->qbuf, (const void*)c->kc[l],
               (const void*)c->vc[l], pos_d, (const unsigned short*)dev->exp_table, c->attn, xq, xd, xisum, n_heads, n_kv, hd,
               seq_cap, seq_cap, pf, (c->qt == CRABML_HIP_Q8_1 ? 1 : 0) | sbit, (long long*)nullptr);
    });
  if (prof) prof_end(dev, &ar);
  return 0;
}

// the tail of the final segment: classifier GEMV over this rank's rows (all of them unless the vocabulary is split,
// llama2.rs:199-208) + greedy sampler + advance.  prof: the classifier launch carries an event pair (stage 5)
int enqueue_classifier_and_sampler(crabml_hip_llama* c, const void* cls_act, bool prof) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const auto& g = c->cfg;
  const int dim = (int)g.embedding_dim;
  int *token_d = c->state, *pos_d = c->state + 1, *step_d = c->state + 2;
  float* out = c->logits + c->vocab_off;
  crabml_hip_device::ProfRec pr{};
  const uint32_t ot = c->output->dtype;
  if (prof)
    CH_TRY(prof_begin(dev, &pr, ot, 5, (double)c->vocab_l * (double)(dim / block_elems(ot)) * (double)block_bytes(ot) + 4.0 * dim + 4.0 * c->vocab_l));
  if (dev->strict_order)
    CH_TRY(launch_gemv_strict(dev, c->output, (size_t)c->vocab_l, dim, cls_act, 1, out));
  else
    CH_TRY(launch_gemv(dev, c->output, (size_t)c->vocab_l, dim, cls_act, 1, out, prof ? &pr : nullptr));
  if (prof) CH_TRY(prof_end(dev, &pr));
  if (c->ext_kv) {
    // a context driven by the recorded-op queue (lazy.hip): the HOST samples (Llama2Runner exports the logits and runs its own
    // sampler, llama2.rs:208), token / position / serial of the next step come from the host (lazy_ctx_begin) -- no sampler launch
    if (c->host_logits != nullptr) {
      const int n = c->vocab_l;
      k_logits_to_host<<<64, 256, 0, st>>>((const f32x4*)out, (f32x4*)c->host_logits, n / 4, out, c->host_logits, n);
      k_host_flag<<<1, 1, 0, st>>>((unsigned*)(c->host_logits + c->cfg.vocab_size), (const int*)(c->state + 7), c->state + 5);
    }
    CH_HIP(dev, hipGetLastError());
    return 0;
  }
  if (c->sampling) {
    const int n = c->vocab_l;
    const SampleStep ss{c->sm_par, c->sm_coins, token_d, pos_d, step_d, c->state + 4, c->out_tokens, c->out_cap, c->state + 5};
    k_sample_max<<<SAMPLE_BLOCKS, 256, 0, st>>>(out, n, c->sm_par, c->sm_bmax);
    k_sample_keys<<<SAMPLE_BLOCKS, 256, 0, st>>>(out, n, c->sm_par, c->sm_bmax, SAMPLE_BLOCKS, (const unsigned short*)dev->exp_table,
                                                 c->sm_keys, c->sm_hist);
    if (dev->strict_order)
      k_sample_pick<true><<<1, SAMPLE_PICK_THREADS, 0, st>>>(c->sm_keys, n, c->sm_hist, ss);
    else
      k_sample_pick<false><<<1, SAMPLE_PICK_THREADS, 0, st>>>(c->sm_keys, n, c->sm_hist, ss);
    CH_HIP(dev, hipGetLastError());
    return 0;
  }
  k_argmax_partial<<<ARGMAX_BLOCKS, 256, 0, st>>>(out, c->vocab_l, c->am_val, c->am_idx, c->vocab_off);
  if (c->split_vocab && c->comm && c->comm->p2p)
    k_argmax_step_tp<<<1, 64, 0, st>>>(c->am_val, c->am_idx, ARGMAX_BLOCKS, token_d, pos_d, step_d, c->out_tokens, c->out_cap, c->state + 4,
                                       tp_view(c, true), n_segments(c));
  else
    k_argmax_step<<<1, 64, 0, st>>>(c->am_val, c->am_idx, ARGMAX_BLOCKS, token_d, pos_d, step_d, c->out_tokens, c->out_cap, c->state + 4,
                                    c->split_vocab ? c->am_best : (int*)nullptr);
  CH_HIP(dev, hipGetLastError());
  return 0;
}

// the q|k|v epilogue arguments of a Qwen2 layer: Llama's plus the layer's three bias vectors
static QkvEpiB qwen2_epi(const crabml_hip_llama* c, const QkvEpi& e, int l) {
  return QkvEpiB{e, (const float*)c->bq[l]->ptr, (const float*)c->bk[l]->ptr, (const float*)c->bv[l]->ptr};
}
template <class E>
struct QkvArchOf {
  static constexpr int value = QKV_LLAMA;
};
template <>
struct QkvArchOf<QkvEpiB> {
  static constexpr int value = QKV_QWEN2;
};
template <>
struct QkvArchOf<QkvEpiN> {
  static constexpr int value = QKV_GEMMA;
};
// f(the epilogue arguments of layer l's q|k|v launch): e itself, Qwen2's, or Gemma's; QkvArchOf<decltype(ep)> is the kernels' ARCH
template <class F>
void with_qkv_epi(const crabml_hip_llama* c, const QkvEpi& e, int l, F&& f) {
  if (c->qwen2)
    f(qwen2_epi(c, e, l));
  else if (c->gemma)
    f(QkvEpiN{e});
  else
    f(e);
}
// what the three segment enqueuers share: the decode step's q|k|v epilogue arguments (rope + scale + KV append, llama2.rs:244-256,
// 542-554, 561-565; local heads only) and the embedding row in front of layer 0
QkvEpi decode_qkv_epi(const crabml_hip_llama* c, int l) {
  return QkvEpi{c->qbuf, c->kc[l], c->vc[l], c->rope, c->state + 1, 1.0f / std::sqrt((float)c->hd), c->dim_l, c->kv_dim_l, c->hd,
                (int)c->cfg.rope_dim, c->npairs, (int)c->cfg.seq_len, c->cfg.use_f16_kv_cache ? 1 : 0};
}
void launch_embed(const crabml_hip_llama* c) {
  const int dim = (int)c->cfg.embedding_dim;
  k_embed<<<(dim + 255) / 256, 256, 0, c->dev->stream>>>((const char*)c->token_embed->ptr, (int)c->token_embed->dtype,
                                                         c->token_embed->wl.off_scale, c->state, dim, c->x, c->embed_scale);
}

// the form <QIN, TP, DEFER> of a k_gemv_res_nq launch, as a value: the caller branches between forms, SPLIT is folded at the launch
template <int QIN, bool TP = false, bool DEFER = false>
struct NqForm {};
// (DEEP, the request depth, is read by the forms whose rhs planes lie in global memory, at one row per wave: QIN 0, SPLIT 2)
template <int FMT, int SPLIT, int DEEP, int QIN, bool TP, bool DEFER>
constexpr auto nq_kernel(NqForm<QIN, TP, DEFER>) {
  return &k_gemv_res_nq<FMT, SPLIT, QIN, TP, DEFER, false, QIN == 0 && SPLIT == 2 ? DEEP : 0>;
}

// enqueue segment `seg` of one decode step on the device stream (see the banner above): the fused kernels
// (fast mode, Q4_0 / Q8_0 weights)
template <int FMT>
int enqueue_segment_t(crabml_hip_llama* c, int seg) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const auto& g = c->cfg;
  const int dim = (int)g.embedding_dim, hd = c->hd;
  const int dim_l = c->dim_l, kv_dim_l = c->kv_dim_l, hidden_l = c->hidden_l;
  const int n_heads_l = c->n_heads_l;
  const bool tp = c->tp > 1;
  const int L = (int)g.n_layers;
  constexpr bool Q81 = rhs_is_q8_1<FMT>;
  // Q5_0 / Q5_1 layers come here on one device only (decide_step): none of the tensor-parallel forms -- k_gateup_h, the f32-rhs
  // prologue, the in-launch collective -- is built for them
  constexpr bool ONE_DEVICE = !has_tp_forms<FMT>;
  if (ONE_DEVICE && c->tp > 1) CH_BAIL(c->dev, CRABML_HIP_UNEXPECTED, "llama: a tensor-parallel rank of a format without tensor-parallel launch forms on the fused segments (decide_step sends it to the per-op segments)");
  const uint32_t qt = c->qt;
  ActPtrs ad = act_ptrs(c->act_dim, dim, qt), aa = act_ptrs(c->act_attn, dim_l, qt), ah = act_ptrs(c->act_hid, hidden_l, qt);
  // measurement hook: only meaningful for eager launches (events cannot live inside the captured graph)
  const bool prof = dev->prof_on && !c->use_graph && !c->capturing;
  const double blk_b = (double)block_bytes(c->wtype) / 32.0;  // weight bytes per element
  auto P0 = [&](crabml_hip_device::ProfRec* r, uint32_t stage, double rows, double k) {
    return prof ? prof_begin(dev, r, c->wtype, stage, rows * k * blk_b + 4.0 * k + 4.0 * rows) : 0;
  };
  auto P1 = [&](crabml_hip_device::ProfRec* r) { return prof ? prof_end(dev, r) : 0; };
  crabml_hip_device::ProfRec pr{};
  crabml_hip_device::ProfRec* R = prof ? &pr : nullptr;
  const bool do_pf = !(g.flags & CRABML_HIP_LLAMA_NO_PREFETCH);
  auto plan = [&](const crabml_hip_buf* a, const crabml_hip_buf* b, const crabml_hip_buf* cc) {
    PrefetchPlan pf{};
    const crabml_hip_buf* v[3] = {a, b, cc};
    for (int i = 0; i < 3; i++) {
      pf.p[i] = do_pf && v[i] ? v[i]->ptr : nullptr;
      pf.n[i] = do_pf && v[i] ? (v[i]->wl.total / 16) * 16 : 0;
    }
    pf.sink = c->state + 3;
    return pf;
  };
  const int spare = do_pf ? (dev->n_cu > 1 ? dev->n_cu - 1 : 0) : 0;
  const size_t norm_lds = norm_lds_bytes(dim);
  // rmsnorm * weight -> act_dim; with tp the previous segment's all-reduced output is folded into x first
  auto norm_quant = [&](const float* wn, float eps, bool add_pending, const PrefetchPlan& pf) {
    crabml_hip_device::ProfRec nr{};
    if (prof) prof_begin(dev, &nr, CRABML_HIP_F32, 6, 8.0 * dim);
    const float* addv = add_pending ? c->partial : nullptr;
    with_const_else<4, 12>(norm_nit(dim), [&](auto nit) {
      launch_k(st, prof ? &nr : nullptr, k_norm_quant<decltype(nit)::value, Q81>, dim3(1 + spare), dim3(1024), norm_lds, c->x, addv, wn, dim, eps, ad.q,
               ad.d, ad.isum, pf, c->plan.ordered ? 0 : 1);
    });
    if (prof) prof_end(dev, &nr);
  };
  // W(dim x k_local) . act -> x (+= residual) or partial (tp)
  const bool norm_epi = c->plan.norm_epi;
  // q / k / v rows of exactly 128 units: both 64-unit steps requested up front (5.29 -> 4.66 us per launch on the 8B shape,
  // profiles/r06_small_stage_ab.md; bit-identical).  A/B hook: CRABML_HIP_TEST_HOOKS=1 CRABML_HIP_QKV_UPFRONT=0 keeps the two rounds.
  static const int qkv_upfront = test_hook_off("CRABML_HIP_QKV_UPFRONT") ? 0 : 1;
  // the hop-free norm between wo and gate/up of a layer: decided once, for the producer and the consumer alike
  const bool defer_wo = c->plan.defer_norm && !Q81;
  // ... and between ffn_down of layer l and q/k/v of layer l + 1 (the last ffn_down feeds the classifier launch: exact planes)
  const bool defer_down = c->plan.defer_norm && !Q81;
  // wnext / eps_next: the RMSNorm that consumes this GEMV's output (norm epilogue only)
  auto gemv_out = [&](const crabml_hip_buf* w, const ActPtrs& a, int k, uint32_t stage, const float* wnext, float eps_next, bool defer = false,
                      const float* xin = nullptr) -> int {
    CH_TRY(P0(&pr, stage, dim, k));
    float* dst = tp ? c->partial : c->x;
    if (norm_epi) {
      NormGather ng{c->slots, c->slots + dim / 16, c->state + 4, c->state + 5, n_segments(c), seg, c->rsums};
      const int split = chunk_split(g.flags, k, dim, dev->n_cu);
      c->tap.note(seg / 2, stage == 2 ? CRABML_HIP_PLAN_SPLIT_WO : CRABML_HIP_PLAN_SPLIT_DOWN, split);
      const TpP2P tpv = tp_view(c, tp);
      // one k_gemv_res_nq launch of the given form: `split` workgroups for each of the dim / 32 chunks, 16 waves each
      const int nwg = dim / 32 * split;
      const int depth = nq_request_depth(g.flags, k, 2 / split, (nwg + dev->n_cu - 1) / dev->n_cu * 16);
      auto nq = [&](auto form, size_t lds, const float* rhs, auto tparg) {
        with_const_else<2, 1>(split, [&](auto s) {
          with_const_else<NQ_DEEP, 0>(depth, [&](auto dp) {
            launch_k(st, R, nq_kernel<FMT, decltype(s)::value, decltype(dp)::value>(form), dim3(nwg), dim3(1024),
                     decltype(dp)::value > 0 && lds == 0 ? q8_0_lds_bytes(k / 32) : lds, planes_of(w), act_view<FMT>(a),
                     rhs, c->x, wnext, eps_next, ad.q, ad.d, ad.isum, ng, k / 32, Planes6{nullptr, 0}, tparg);
          });
        });
      };
      if (xin != nullptr && !Q81 && !ONE_DEVICE) {  // (tensor-parallel ranks) the rhs arrives as f32 -- h from k_gateup_h -- and is quantized in the prologue
        if constexpr (!Q81 && !ONE_DEVICE) {
          if (tpv.n > 1)
            nq(NqForm<1, true>{}, q8_0_lds_bytes(k / 32), xin, tpv);
          else
            nq(NqForm<1>{}, q8_0_lds_bytes(k / 32), xin, NoTp{});
        }
      } else if (tpv.n > 1 && !ONE_DEVICE) {  // tensor parallel over a P2P group: the collective runs inside this launch
        if constexpr (!ONE_DEVICE) nq(NqForm<0, true>{}, 0, nullptr, tpv);
      } else if (c->plan.ordered) {  // strict order: the same launch with block-ordered GEMV sums and the reference's norm order
        // tuning hook: 0 = never, 1 = ffn_down only, 2 = wo too (-1 / unset: the default below)
        static const int pipe_mode = test_hook_int("CRABML_HIP_ORD_PIPE", -1);
        // measured (profiles/r04_strict_order_decode.md): the pipelined chain pays in ffn_down for every format, in wo for Q8_0 only
        const int pipe = pipe_mode >= 0 ? pipe_mode : FMT == CRABML_HIP_Q8_0 ? 2 : 1;
        const bool piped = pipe >= (split == 2 ? 1 : 2);  // (two workgroups per chunk: ffn_down)
        with_const_else<2, 1>(split, [&](auto s) {
          with_const_else<0, 1>(piped, [&](auto p) {
            launch_k(st, R, k_gemv_res_nq_ord<FMT, decltype(s)::value, decltype(p)::value != 0>, dim3(dim / 32 * split), dim3(1024),
                     nq_ord_lds_bytes(k / 32, split), planes_of(w), act_view<FMT>(a), c->x, wnext, eps_next, ad.q, ad.d, ad.isum, ng, k / 32);
          });
        });
      } else if (defer && !Q81) {  // hop-free: the consumer applies 1 / rms
        if constexpr (!Q81) nq(NqForm<0, false, true>{}, 0, nullptr, NoTp{});
      } else {
        nq(NqForm<0>{}, 0, nullptr, NoTp{});
      }
    } else if (c->plan.ordered) {
      launch_k(st, R, k_gemv_res_ord<FMT>, dim3((dim + 7) / 8), dim3(256), ord_terms_lds_bytes(k / 32), planes_of(w), act_view<FMT>(a), c->x, dim, k / 32);
    } else if (tp && !ONE_DEVICE) {
      if constexpr (!ONE_DEVICE)
        launch_k(st, R, k_gemv_res<FMT, 1, false>, dim3((dim + 1) / 2), dim3(128), 0, planes_of(w), act_view<FMT>(a), dst, dim, k / 32);
    } else {
      launch_k(st, R, k_gemv_res<FMT, 1, true>, dim3((dim + 1) / 2), dim3(128), 0, planes_of(w), act_view<FMT>(a), dst, dim, k / 32);
    }
    CH_TRY(P1(&pr));
    return 0;
  };

  // the tap (test hook): host-side copies between the launches of the tapped layer; a no-op unless a tapped step is being enqueued
  const size_t ad_bytes = act_layout(qt, (size_t)dim).total, rs_bytes = c->rsums ? (size_t)(dim / 32) * 4 : 0;
  TapRec& tap = c->tap;
  auto TAP = [&](bool on, int f, const void* src, size_t bytes) -> int { return on ? tap.copy(c, f, src, bytes) : 0; };
  if (seg == 2 * L) {  // final rmsnorm + classifier (llama2.rs:274-278, 199-208) + greedy sampler
    const void* cls_act = c->act_dim;
    if (c->out_qt != qt) {
      // the classifier has its own rhs type (e.g. Q6_K -> Q8_K): normalize the final x to f32 and quantize for it (the
      // planes the last ffn_down epilogue wrote are in the layers' type and stay unused)
      const float* addv = tp && !norm_epi ? c->partial : nullptr;  // (fused collective: x is already final)
      launch_norm_f32(st, c->x, addv, (const float*)c->rms_final->ptr, dim, g.rms_norm_eps, c->xn, c->plan.ordered ? 0 : 1);
      if (c->out_qt == CRABML_HIP_F32) {
        cls_act = c->xn;
      } else {
        launch_quantize_act(st, c->out_qt, c->xn, (size_t)dim, c->act_dim);
      }
    } else if (!norm_epi) {
      norm_quant((const float*)c->rms_final->ptr, g.rms_norm_eps, tp, plan(nullptr, nullptr, nullptr));
      CH_TRY(TAP(tap.layer == L - 1, CRABML_HIP_TAP_DOWN_ACT, c->act_dim, ad_bytes));
    }
    CH_TRY(TAP(true, CRABML_HIP_TAP_CLS_ACT, cls_act, c->out_qt == CRABML_HIP_F32 ? (size_t)dim * 4 : act_layout(c->out_qt, (size_t)dim).total));
    return enqueue_classifier_and_sampler(c, cls_act, prof);
  }
  const int l = seg / 2;
  if ((seg & 1) == 0) {
    if (l == 0) launch_embed(c);
    // attention rmsnorm (llama2.rs:230-234)
    if (!norm_epi || l == 0)
      norm_quant((const float*)c->rms_att[l]->ptr, g.rms_norm_eps, tp && l > 0, plan(c->wq[l], c->wk[l], c->wv[l]));
    const bool tl = tap.layer == l;
    if (!norm_epi || l == 0) tap.note(l, CRABML_HIP_PLAN_NORM_NIT, norm_nit(dim));
    CH_TRY(TAP(!norm_epi && l > 0 && tap.layer == l - 1, CRABML_HIP_TAP_DOWN_ACT, c->act_dim, ad_bytes));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_QKV_IN_X, c->x, (size_t)dim * 4));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_QKV_IN_ACT, c->act_dim, ad_bytes));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_QKV_IN_RSUMS, c->rsums, rs_bytes));
    // q, k, v + rope + scale + KV append, local heads only
    const QkvEpi e = decode_qkv_epi(c, l);
    const int total_rows = dim_l + 2 * kv_dim_l;
    CH_TRY(P0(&pr, 1, total_rows, dim));
    // (the planes of layer l > 0 come from the previous layer's ffn_down launch, with its dim / 32 chunk sums)
    const RmsTail rtq{c->rsums, dim / 32, 1.0f / (float)dim, g.rms_norm_eps};
    // the two arguments that pick k_qkv's loader: DEFER (1 / rms applied here) and `upfront` -- without DEFER only for few, short
    // waves (a tensor-parallel rank's rows; small models): two steps per request round
    const bool deferq = defer_down && l > 0;  // (defer_down: never Q4_1)
    const int upfront = deferq ? qkv_upfront : (qkv_upfront && total_rows / 2 <= 4 * dev->n_cu) ? 1 : 0;
    if (!c->plan.ordered) {  // (what the kernel makes of them: rows_partial_rms / rows_partial, gemv_core.hpp)
      const int nu = dim / 32 * BlockFmt<FMT>::UNITS;
      tap.note(l, CRABML_HIP_PLAN_QKV_LOADER, deferq ? (upfront && nu == 128 ? 4 : 3) : (upfront && nu % 128 == 0 ? 2 : 1));
    }
    with_qkv_epi(c, e, l, [&](auto ep) {
      constexpr int A = QkvArchOf<decltype(ep)>::value;
      if (c->plan.ordered)
        launch_k(st, R, k_qkv_ord<FMT, A>, dim3((total_rows / 2 + 3) / 4), dim3(256), ord_terms_lds_bytes(dim / 32), planes_of(c->wq[l]),
                 planes_of(c->wk[l]), planes_of(c->wv[l]), act_view<FMT>(ad), dim / 32, ep, Planes6{nullptr, 0});
      else if (deferq) {
        if constexpr (!Q81)
          launch_k(st, R, k_qkv<FMT, true, A>, dim3((total_rows / 2 + 1) / 2), dim3(128), 0, planes_of(c->wq[l]), planes_of(c->wk[l]),
                   planes_of(c->wv[l]), act_view<FMT>(ad), dim / 32, ep, Planes6{nullptr, 0}, rtq, upfront);
      } else
        launch_k(st, R, k_qkv<FMT, false, A>, dim3((total_rows / 2 + 1) / 2), dim3(128), 0, planes_of(c->wq[l]), planes_of(c->wk[l]),
                 planes_of(c->wv[l]), act_view<FMT>(ad), dim / 32, ep, Planes6{nullptr, 0}, rtq, upfront);
    });
    CH_TRY(P1(&pr));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_QBUF, c->qbuf, (size_t)dim_l * 4));
    // attention (llama2.rs:571-590) -> attn (f32) [+ Q8_0 planes for wo]; spare CUs prefetch wo
    const bool attn_quant = (hd % 32) == 0;
    const int attn_spare = do_pf && dev->n_cu > n_heads_l ? dev->n_cu - n_heads_l : 0;
    CH_TRY(enqueue_attention(c, l, attn_quant ? aa.q : (signed char*)nullptr, aa.d, aa.isum, plan(c->wo[l], nullptr, nullptr), attn_spare, prof));
    if (!attn_quant) launch_quantize_act(st, qt, c->attn, (size_t)dim_l, c->act_attn);
    CH_TRY(TAP(tl, CRABML_HIP_TAP_ATTN, c->attn, (size_t)dim_l * 4));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_ACT_ATTN, c->act_attn, act_layout(qt, (size_t)dim_l).total));
    // wo (+ residual, llama2.rs:600, 266): k = the local heads' slice
    CH_TRY(gemv_out(c->wo[l], aa, dim_l, 2, (const float*)c->rms_ffn[l]->ptr, 1e-5f, defer_wo));
  } else {
    // ffn rmsnorm, eps = the literal 1e-5 (llama2.rs:611)
    if (!norm_epi) norm_quant((const float*)c->rms_ffn[l]->ptr, 1e-5f, tp, plan(nullptr, nullptr, nullptr));
    const bool tl = tap.layer == l;
    CH_TRY(TAP(tl, CRABML_HIP_TAP_WO_X, c->x, (size_t)dim * 4));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_WO_ACT, c->act_dim, ad_bytes));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_WO_RSUMS, c->rsums, rs_bytes));
    const float* wnext_down = (const float*)(l + 1 < L ? c->rms_att[l + 1] : c->rms_final)->ptr;
    // gate / up + silu * mul (llama2.rs:620-630), local rows
    CH_TRY(P0(&pr, 3, 2.0 * hidden_l, dim));
    const RmsTail rt{c->rsums, dim / 32, 1.0f / (float)dim, 1e-5f};  // eps: the literal 1e-5 (llama2.rs:611)
    const bool hq = c->plan.gu_rows > 0 && !c->plan.ordered && norm_epi && !Q81 && !ONE_DEVICE && !defer_wo;
    if (hq) {
      if constexpr (!Q81 && !ONE_DEVICE)
        launch_k(st, R, k_gateup_h<FMT>, dim3(hidden_l / c->plan.gu_rows), dim3(c->plan.gu_rows / 2 * 64), 0, planes_of(c->gate[l]), planes_of(c->up[l]),
                 act_view<FMT>(ad), c->ffn_act, c->h, hidden_l, dim / 32);
    } else if (c->plan.ordered)
      launch_k(st, R, k_gateup_q_ord<FMT>, dim3(hidden_l / 32), dim3(1024), gateup_q_ord_lds_bytes(dim / 32), planes_of(c->gate[l]),
               planes_of(c->up[l]), act_view<FMT>(ad), c->ffn_act, ah.q, ah.d, ah.isum, dim / 32);
    else if (defer_wo) {
      if constexpr (!Q81)
        launch_k(st, R, k_gateup_q<FMT, true>, dim3(hidden_l / 32), dim3(1024), 0, planes_of(c->gate[l]), planes_of(c->up[l]), act_view<FMT>(ad),
                 c->ffn_act, ah.q, ah.d, ah.isum, dim / 32, rt);
    } else
      launch_k(st, R, k_gateup_q<FMT>, dim3(hidden_l / 32), dim3(1024), 0, planes_of(c->gate[l]), planes_of(c->up[l]),
               act_view<FMT>(ad), c->ffn_act, ah.q, ah.d, ah.isum, dim / 32, rt);
    CH_TRY(P1(&pr));
    CH_TRY(TAP(tl && !hq, CRABML_HIP_TAP_ACT_HID, c->act_hid, act_layout(qt, (size_t)hidden_l).total));
    // down (+ residual, llama2.rs:633-636): k = the local hidden slice
    CH_TRY(gemv_out(c->down[l], ah, hidden_l, 4, wnext_down, g.rms_norm_eps, defer_down && l + 1 < L, hq ? c->h : nullptr));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_DOWN_X, c->x, (size_t)dim * 4));
    CH_TRY(TAP(tl && norm_epi, CRABML_HIP_TAP_DOWN_ACT, c->act_dim, ad_bytes));
    CH_TRY(TAP(tl && norm_epi, CRABML_HIP_TAP_DOWN_RSUMS, c->rsums, rs_bytes));
  }
  CH_HIP(dev, hipGetLastError());
  return 0;
}

// The same segment out of per-op launches: one GEMV launch per weight matrix (any format matmul_vec supports;
// the rhs is quantized to vec_dot_rhs_dtype(weight), buf/api.rs:142-159) plus small epilogue kernels.  Used by
// the strict-order device (scalar summation order, bit-exact against the oracle for every format) and, in fast
// mode, by the formats without fused kernels (Q4_1, Q4_K, Q8_K, F16, F32).  Still one hipGraph per step.
int enqueue_segment_generic(crabml_hip_llama* c, int seg) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const auto& g = c->cfg;
  const int dim = (int)g.embedding_dim;
  const int dim_l = c->dim_l, kv_dim_l = c->kv_dim_l, hidden_l = c->hidden_l;
  const bool strict = dev->strict_order;
  const bool tp = c->tp > 1;
  const int L = (int)g.n_layers;
  const bool prof = dev->prof_on && !c->use_graph && !c->capturing && !strict;
  crabml_hip_device::ProfRec pr{};
  auto gemv = [&](const crabml_hip_buf* w, int m, int k, const void* act, float* out, uint32_t stage) -> int {
    if (strict) return launch_gemv_strict(dev, w, m, k, act, 1, out);
    if (prof)
      CH_TRY(prof_begin(dev, &pr, w->dtype, stage,
                        (double)m * (double)(k / block_elems(w->dtype)) * (double)block_bytes(w->dtype) + 4.0 * k + 4.0 * m));
    CH_TRY(launch_gemv(dev, w, m, k, act, 1, out, prof ? &pr : nullptr));
    if (prof) CH_TRY(prof_end(dev, &pr));
    return 0;
  };
  // CpuTensorBuf::quantize for the rhs of matmul_vec: F32 is the vector itself
  auto quant = [&](const float* src, int n, uint32_t qt, char* planes) -> const void* {
    if (qt == CRABML_HIP_F32) return src;
    launch_quantize_act(st, qt, src, (size_t)n, planes);
    return planes;
  };
  auto norm = [&](const float* wn, float eps, bool add_pending) {
    launch_norm_f32(st, c->x, add_pending ? c->partial : nullptr, wn, dim, eps, c->xn, strict ? 0 : 1);
  };
  float* dst = tp ? c->partial : c->x;

  if (seg == 2 * L) {
    norm((const float*)c->rms_final->ptr, g.rms_norm_eps, tp);
    const void* act = quant(c->xn, dim, c->out_qt, c->act_dim);
    return enqueue_classifier_and_sampler(c, act, prof);
  }
  const int l = seg / 2;
  if ((seg & 1) == 0) {
    if (l == 0) launch_embed(c);
    norm((const float*)c->rms_att[l]->ptr, g.rms_norm_eps, tp && l > 0);
    const void* act = quant(c->xn, dim, c->qt, c->act_dim);
    const int total_rows = dim_l + 2 * kv_dim_l;
    CH_TRY(gemv(c->wq[l], dim_l, dim, act, c->tmp, 1));
    CH_TRY(gemv(c->wk[l], kv_dim_l, dim, act, c->tmp + dim_l, 1));
    CH_TRY(gemv(c->wv[l], kv_dim_l, dim, act, c->tmp + dim_l + kv_dim_l, 1));
    with_qkv_epi(c, decode_qkv_epi(c, l), l, [&](auto ep) {
      k_qkv_epi<QkvArchOf<decltype(ep)>::value><<<(total_rows / 2 + 255) / 256, 256, 0, st>>>(c->tmp, ep);
    });
    CH_TRY(enqueue_attention(c, l, nullptr, nullptr, nullptr, PrefetchPlan{}, 0, prof));
    const void* aact = quant(c->attn, dim_l, c->qt, c->act_attn);
    if (strict && !tp) {  // the residual inside the GEMV's own store: x = matmul_out + x (llama2.rs:266)
      CH_TRY(launch_gemv_strict(dev, c->wo[l], dim, dim_l, aact, 1, c->x, c->x));
    } else {
      CH_TRY(gemv(c->wo[l], dim, dim_l, aact, c->tmp, 2));
      k_res_epi<<<(dim + 255) / 256, 256, 0, st>>>(c->tmp, dst, dim, tp ? 0 : 1);
    }
  } else {
    norm((const float*)c->rms_ffn[l]->ptr, 1e-5f, tp);  // llama2.rs:611
    const void* act = quant(c->xn, dim, c->qt, c->act_dim);
    CH_TRY(gemv(c->gate[l], hidden_l, dim, act, c->tmp, 3));
    CH_TRY(gemv(c->up[l], hidden_l, dim, act, c->tmp + hidden_l, 3));
    k_gateup_epi<<<(hidden_l + 255) / 256, 256, 0, st>>>(c->tmp, c->tmp + hidden_l, c->ffn_act, c->h, hidden_l);
    const void* hact = quant(c->h, hidden_l, c->qt, c->act_hid);
    if (strict && !tp) {
      CH_TRY(launch_gemv_strict(dev, c->down[l], dim, hidden_l, hact, 1, c->x, c->x));
    } else {
      CH_TRY(gemv(c->down[l], dim, hidden_l, hact, c->tmp, 4));
      k_res_epi<<<(dim + 255) / 256, 256, 0, st>>>(c->tmp, dst, dim, tp ? 0 : 1);
    }
  }
  CH_HIP(dev, hipGetLastError());
  return 0;
}

// K-quant bodies (KBodies above) and Q4_1 layers (fast mode): the fused GEMV kernels with the format's inner loop against Q8_K / Q8_1
// activation planes.  The rhs quantizer is its own launch here (a Q8_K super-block spans 256 rows: eight 32-row
// workgroups; Q8_1 keeps the same structure), so a layer is 11 launches instead of the per-op path's 18.
template <int FMT>
int enqueue_segment_k(crabml_hip_llama* c, int seg) {
  // a K-quant body: the same five launches with the format's own row loader (its policy, KBody); an EPI_ONLY body is built in the
  // norm-epilogue form only (decide_step).  A body whose alternates do not come whole (V_WHOLE false: the Q3_K and the Q2_K recipe
  // families) has attn_v, attn_output and ffn_down each in its own format or one of VAlt: wo and ffn_down are launched with the
  // instantiation of the TENSOR's format, the V rows take k_qkv's hand-over.
  constexpr bool KF = KBody<FMT>::IS, EPI_ONLY = KBody<FMT>::EPI_ONLY;
  constexpr uint32_t QT = KF ? CRABML_HIP_Q8_K : CRABML_HIP_Q8_1;
  constexpr int BE = KF ? 256 : 32;  // elements per weight block
  typedef typename ActOf<FMT>::type Act;
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const auto& g = c->cfg;
  const int dim = (int)g.embedding_dim;
  const int dim_l = c->dim_l, kv_dim_l = c->kv_dim_l, hidden_l = c->hidden_l;
  const bool tp = c->tp > 1;
  const int L = (int)g.n_layers;
  const bool prof = dev->prof_on && !c->use_graph && !c->capturing;
  crabml_hip_device::ProfRec pr{};
  crabml_hip_device::ProfRec* R = prof ? &pr : nullptr;
  const double blk_b = (double)block_bytes(FMT) / (double)BE;
  auto P0 = [&](uint32_t stage, double rows, double k) {
    return prof ? prof_begin(dev, &pr, FMT, stage, rows * k * blk_b + 4.0 * k + 4.0 * rows) : 0;
  };
  auto P1 = [&]() { return prof ? prof_end(dev, &pr) : 0; };
  auto act_k = [&](char* planes, int n) { return act_at<Act>(planes, act_layout(QT, (size_t)n)); };
  // a Q6_K tensor inside a layer whose body takes it whole (attn_v / ffn_down of the *_K_M mixes): handed to the kernel beside the planes
  // (no other body ever holds one beside its own format: validate_weights)
  auto six = [&](const crabml_hip_buf* b) {
    return kbody_takes_q6k<FMT> && b->dtype == CRABML_HIP_Q6_K ? Planes6{(const char*)b->ptr, b->wl.off_scale} : Planes6{nullptr, 0};
  };
  // ... and what the V matrix hands k_qkv (VOther, fused_common.hpp): its format where the alternates do not come whole
  auto v_other = [&](const crabml_hip_buf* b) {
    if constexpr (!KBody<FMT>::V_WHOLE)
      return VFormat{(int)b->dtype};
    else
      return six(b);
  };
  // rmsnorm * weight -> xn -> Q8_K planes (buf_q8_k.rs:84-131)
  auto norm_quant = [&](const float* wn, float eps, bool add_pending, uint32_t qt) -> const void* {
    launch_norm_f32(st, c->x, add_pending ? c->partial : nullptr, wn, dim, eps, c->xn, c->plan.ordered ? 0 : 1);
    if (qt == CRABML_HIP_F32) return c->xn;
    launch_quantize_act(st, qt, c->xn, (size_t)dim, c->act_dim);
    return c->act_dim;
  };
  float* dst = tp ? c->partial : c->x;
  const bool nepi = KF && c->plan.norm_epi_k;
  // strict-order device, Q4_K layers (c->plan.ordered): the same five launches with every sum in the reference's order -- nine-term records per
  // super-block added in order (q4k_class_terms / q4k_ordered_sum, gemv_core.hpp), the reference's norm order in the epilogue
  const bool ordk = FMT == CRABML_HIP_Q4_K && c->plan.ordered;
  // wnext / eps_next: the RMSNorm that consumes this GEMV's output (norm epilogue only)
  // the rhs of wo / ffn_down quantized by the consuming kernel itself (no quantizer launch)
  const bool qin = nepi && !(g.flags & CRABML_HIP_LLAMA_NO_RHS_PROLOGUE) && dim_l % 256 == 0 && hidden_l % 256 == 0;
  const bool qout = qin && c->plan.q8k_producers;  // attention / gate-up write the planes, wo / ffn_down copy them
  // wo leaves x and its chunk sums only -- wo_parts per 32-row chunk -- and gate | up runs its NORMIN form: one value for the wo launch,
  // the gate | up launch and the tap (k_norm_in is never set on a strict-order device: decide_step)
  const bool wo_x_only = !ordk && qout && c->plan.k_norm_in;
  const int wo_parts = wo_x_only ? chunk_split(g.flags, dim_l, dim, dev->n_cu, true) : 1;
  // wnext / eps_next: the RMSNorm that consumes this GEMV's output (norm epilogue only); xin: the f32 rhs
  // qmode: 0 = rhs planes from global memory, 1 = quantize the f32 rhs in the kernel's prologue, 2 = copy finished planes
  auto gemv_out = [&](const crabml_hip_buf* w, const Act& a, const float* xin, int k, uint32_t stage, const float* wnext,
                      float eps_next, int qmode, bool x_only = false) -> int {
    CH_TRY(P0(stage, dim, k));
    if constexpr (KF) {
      if (nepi) {
        NormGather ng{c->slots, c->slots + dim / 16, c->state + 4, c->state + 5, n_segments(c), seg, c->rsums};
        ActLayout al = act_layout(QT, (size_t)dim);
        ng.qp = (signed char*)(c->act_dim + al.off_p);
        signed char* oq = x_only ? nullptr : (signed char*)c->act_dim;  // (x_only: the consumer quantizes, nq_epilogue)
        void* od = (void*)(c->act_dim + al.off_d);
        void* ob = (void*)(c->act_dim + al.off_aux);
        const int split = chunk_split(g.flags, k, dim, dev->n_cu, x_only);
        c->tap.note(seg / 2, stage == 2 ? CRABML_HIP_PLAN_SPLIT_WO : CRABML_HIP_PLAN_SPLIT_DOWN, split);
        c->tap.note(seg / 2, stage == 2 ? CRABML_HIP_PLAN_QMODE_WO : CRABML_HIP_PLAN_QMODE_DOWN, qmode);
        if (stage == 2) c->tap.note(seg / 2, CRABML_HIP_PLAN_WO_X_ONLY, x_only ? 1 : 0);
        if constexpr (!EPI_ONLY)
          if (ordk) {  // (qmode is 1 or 2 here: `qin` holds on every ordered context)
            launch_k(st, R, nq_ord_k_kernel(split, qmode == 2 ? 2 : 1), dim3(dim / 32 * split), dim3(1024), q8k_ord_lds_bytes(k, 32 / split), planes_of(w),
                     a, xin, c->x, wnext, eps_next, oq, od, ob, ng, k / BE, six(w), NoTp{});
            return P1();
          }
        // the instantiation: the body's -- or the tensor's own (the body's format or one of its VAlt: validate_weights) where the
        // alternates do not come whole
        auto launch_nq = [&](auto wf) {
          with_const_else<2, 1>(split, [&](auto s) {
            with_const_else<2, 1, 0>(qmode, [&](auto q) {  // (the rhs planes in LDS unless they are read from global memory)
              launch_k(st, R, k_gemv_res_nq<decltype(wf)::value, decltype(s)::value, decltype(q)::value>, dim3(dim / 32 * split), dim3(1024),
                       qmode ? q8k_lds_bytes(k) : 0, planes_of(w), a, xin, c->x, wnext, eps_next, oq, od, ob, ng, k / BE, six(w), NoTp{});
            });
          });
        };
        if constexpr (!KBody<FMT>::V_WHOLE)
          with_body_or_alt<FMT>(typename KBody<FMT>::VAlt{}, (int)w->dtype, launch_nq);
        else
          launch_nq(std::integral_constant<int, FMT>{});
        return P1();
      }
    }
    if constexpr (EPI_ONLY) {
      CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a K-quant body that exists in the norm-epilogue form only, outside it (decide_step sends it to the per-op segments)");
    } else {
      if (tp)
        launch_k(st, R, k_gemv_res<FMT, 1, false>, dim3((dim + 1) / 2), dim3(128), 0, planes_of(w), a, dst, dim, k / BE);
      else
        launch_k(st, R, k_gemv_res<FMT, 1, true>, dim3((dim + 1) / 2), dim3(128), 0, planes_of(w), a, dst, dim, k / BE);
      return P1();
    }
  };

  // the tap (test hook): host-side copies between the launches of the tapped layer; a no-op unless a tapped step is being enqueued.
  // A set of planes is copied where a launch wrote it to global memory, a Q8_K set's class-major plane as a field of its own.
  TapRec& tap = c->tap;
  auto TAP = [&](bool on, int f, const void* src, size_t bytes) -> int { return on ? tap.copy(c, f, src, bytes) : 0; };
  auto TAPQ = [&](bool on, int f, int f_qp, const void* planes, uint32_t qt, int n) -> int {
    if (!on) return 0;
    const ActLayout al = act_layout(qt, (size_t)n);
    CH_TRY(tap.copy(c, f, planes, qt == CRABML_HIP_F32 ? (size_t)n * 4 : al.total));
    if (qt == CRABML_HIP_Q8_K) CH_TRY(tap.copy(c, f_qp, (const char*)planes + al.off_p, (size_t)n));
    return 0;
  };
  tap.note(CRABML_HIP_PLAN_QIN, qin ? 1 : 0);
  if (seg == 2 * L) {
    const void* act = nepi ? (const void*)c->act_dim : norm_quant((const float*)c->rms_final->ptr, g.rms_norm_eps, tp, c->out_qt);
    CH_TRY(TAP(!nepi, CRABML_HIP_TAP_CLS_XN, c->xn, (size_t)dim * 4));
    CH_TRY(TAPQ(true, CRABML_HIP_TAP_CLS_ACT, CRABML_HIP_TAP_CLS_QP, act, c->out_qt, dim));
    return enqueue_classifier_and_sampler(c, act, prof);
  }
  const int l = seg / 2;
  const bool tl = tap.layer == l;
  if ((seg & 1) == 0) {
    if (l == 0) launch_embed(c);
    if (!nepi || l == 0) norm_quant((const float*)c->rms_att[l]->ptr, g.rms_norm_eps, tp && l > 0, QT);
    CH_TRY(TAP(tl && (!nepi || l == 0), CRABML_HIP_TAP_QKV_IN_XN, c->xn, (size_t)dim * 4));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_QKV_IN_X, c->x, (size_t)dim * 4));
    CH_TRY(TAPQ(tl, CRABML_HIP_TAP_QKV_IN_ACT, CRABML_HIP_TAP_QKV_IN_QP, c->act_dim, QT, dim));
    tap.note(l, CRABML_HIP_PLAN_V_Q6K, c->wv[l]->dtype == CRABML_HIP_Q6_K ? 1 : 0);
    const int total_rows = dim_l + 2 * kv_dim_l;
    CH_TRY(P0(1, total_rows, dim));
    with_qkv_epi(c, decode_qkv_epi(c, l), l, [&](auto ep) {
      constexpr int A = QkvArchOf<decltype(ep)>::value;
      if constexpr (!EPI_ONLY)
        if (ordk) {
          launch_k(st, R, k_qkv_ord<FMT, A>, dim3((total_rows / 2 + 3) / 4), dim3(256), ord_terms_k_lds_bytes(dim / BE), planes_of(c->wq[l]),
                   planes_of(c->wk[l]), planes_of(c->wv[l]), act_k(c->act_dim, dim), dim / BE, ep, six(c->wv[l]));
          return;
        }
      launch_k(st, R, k_qkv<FMT, false, A>, dim3((total_rows / 2 + 1) / 2), dim3(128), 0, planes_of(c->wq[l]), planes_of(c->wk[l]),
               planes_of(c->wv[l]), act_k(c->act_dim, dim), dim / BE, ep, v_other(c->wv[l]), RmsTail{nullptr, 0, 0.f, 0.f}, 0);
    });
    CH_TRY(P1());
    CH_TRY(TAP(tl, CRABML_HIP_TAP_QBUF, c->qbuf, (size_t)dim_l * 4));
    // Q8_K producers: the (short-context) attention kernel assembles the planes of wo's rhs itself; wo copies them
    const bool aq8 = qout && (g.flags & CRABML_HIP_LLAMA_Q8K_ATTN_PRODUCER) && c->attn_variant == 0 && c->plan.attn_s_rows > 0;
    tap.note(l, CRABML_HIP_PLAN_AQ8, aq8 ? 1 : 0);
    if constexpr (KF) {
      if (aq8) {
        const ActLayout ala = act_layout(QT, (size_t)dim_l);
        const AttnQ8K k8{Q8KExchange{c->a8gran, c->state + 4, c->state + 5, n_segments(c), seg}, (float*)(c->act_attn + ala.off_d),
                         (short*)(c->act_attn + ala.off_aux), (signed char*)(c->act_attn + ala.off_p)};
        CH_TRY(enqueue_attention(c, l, (signed char*)c->act_attn, nullptr, nullptr, PrefetchPlan{}, 0, prof, &k8));
      } else {
        CH_TRY(enqueue_attention(c, l, nullptr, nullptr, nullptr, PrefetchPlan{}, 0, prof));
      }
    } else {
      CH_TRY(enqueue_attention(c, l, nullptr, nullptr, nullptr, PrefetchPlan{}, 0, prof));
    }
    if (!qin) launch_quantize_act(st, QT, c->attn, (size_t)dim_l, c->act_attn);
    CH_TRY(TAP(tl, CRABML_HIP_TAP_ATTN, c->attn, (size_t)dim_l * 4));
    CH_TRY(TAPQ(tl && (aq8 || !qin), CRABML_HIP_TAP_ACT_ATTN, CRABML_HIP_TAP_ACT_ATTN_QP, c->act_attn, QT, dim_l));  // (else: wo's prologue quantizes)
    CH_TRY(gemv_out(c->wo[l], act_k(c->act_attn, dim_l), c->attn, dim_l, 2, (const float*)c->rms_ffn[l]->ptr, 1e-5f, aq8 ? 2 : qin ? 1 : 0,
                    wo_x_only));
  } else {
    if (!nepi) norm_quant((const float*)c->rms_ffn[l]->ptr, 1e-5f, tp, QT);  // llama2.rs:611
    // what gate | up reads: wo left x and its chunk sums only (the NORMIN form below), or planes in global memory
    CH_TRY(TAP(tl && !nepi, CRABML_HIP_TAP_WO_XN, c->xn, (size_t)dim * 4));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_WO_X, c->x, (size_t)dim * 4));
    CH_TRY(TAPQ(tl && !wo_x_only, CRABML_HIP_TAP_WO_ACT, CRABML_HIP_TAP_WO_QP, c->act_dim, QT, dim));
    CH_TRY(TAP(tl && wo_x_only, CRABML_HIP_TAP_WO_RSUMS, c->rsums, (size_t)(dim / 32) * wo_parts * 4));
    tap.note(l, CRABML_HIP_PLAN_DOWN_Q6K, c->down[l]->dtype == CRABML_HIP_Q6_K ? 1 : 0);
    CH_TRY(P0(3, 2.0 * hidden_l, dim));
    if constexpr (KF) {
      const ActLayout alh = act_layout(QT, (size_t)hidden_l);
      const Q8KExchange hx{c->h8gran, c->state + 4, c->state + 5, n_segments(c), seg};
      // the form <QOUT, ORD, NORMIN>: h leaves as Q8_K planes too / strict order / wo left x only (above) and this launch normalizes
      // and quantizes the row itself from wo's chunk sums, as many per chunk as wo had workgroups
      const bool normin = wo_x_only;
      char* const hp = qout ? c->act_hid : nullptr;  // (no planes without QOUT; hidden_l % 32 == 0: llama_create_impl)
      const float *nx = nullptr, *nw = nullptr, *nsums = nullptr;
      int sum_parts = 1;
      if (normin) {
        nx = c->x;
        nw = (const float*)c->rms_ffn[l]->ptr;
        nsums = c->rsums;
        sum_parts = wo_parts;
      }
      launch_k(st, R, gateup_k_kernel(qout, ordk, normin, KF ? FMT : CRABML_HIP_Q4_K), dim3(hidden_l / 32), dim3(1024), ordk ? q8k_ord_lds_bytes(dim, 64) : q8k_lds_bytes(dim),
               planes_of(c->gate[l]), planes_of(c->up[l]), act_k(c->act_dim, dim), c->ffn_act, c->h, hidden_l, dim / 256, hx,
               (signed char*)hp, (float*)(hp ? hp + alh.off_d : nullptr), (short*)(hp ? hp + alh.off_aux : nullptr),
               (signed char*)(hp ? hp + alh.off_p : nullptr), nx, nw, normin ? 1e-5f : 0.f, nsums, sum_parts);
    } else {
      launch_k(st, R, k_gateup<FMT>, dim3((hidden_l + 1) / 2), dim3(128), 0, planes_of(c->gate[l]), planes_of(c->up[l]),
               act_k(c->act_dim, dim), c->ffn_act, c->h, hidden_l, dim / BE);
    }
    CH_TRY(P1());
    if (!qin) launch_quantize_act(st, QT, c->h, (size_t)hidden_l, c->act_hid);
    CH_TRY(TAP(tl, CRABML_HIP_TAP_GATEUP_H, c->h, (size_t)hidden_l * 4));
    CH_TRY(TAPQ(tl && (qout || !qin), CRABML_HIP_TAP_ACT_HID, CRABML_HIP_TAP_ACT_HID_QP, c->act_hid, QT, hidden_l));  // (else: ffn_down's prologue quantizes)
    CH_TRY(gemv_out(c->down[l], act_k(c->act_hid, hidden_l), c->h, hidden_l, 4,
                    (const float*)(l + 1 < L ? c->rms_att[l + 1] : c->rms_final)->ptr, g.rms_norm_eps, qout ? 2 : qin ? 1 : 0));
    CH_TRY(TAP(tl, CRABML_HIP_TAP_DOWN_X, c->x, (size_t)dim * 4));
    CH_TRY(TAPQ(tl && nepi, CRABML_HIP_TAP_DOWN_ACT, CRABML_HIP_TAP_DOWN_QP, c->act_dim, QT, dim));
  }
  CH_HIP(dev, hipGetLastError());
  return 0;
}

int enqueue_segment(crabml_hip_llama* c, int seg) {
  switch (c->plan.path) {
    case SegPath::FusedK:
    {
      int rc = 0;
      if (with_fmt(KBodies{}, (int)c->wtype, [&](auto body) { rc = enqueue_segment_k<decltype(body)::value>(c, seg); })) return rc;
      return c->wtype == CRABML_HIP_Q5_1 ? enqueue_segment_k<CRABML_HIP_Q5_1>(c, seg) : enqueue_segment_k<CRABML_HIP_Q4_1>(c, seg);
    }
    case SegPath::Fused5:
      return c->wtype == CRABML_HIP_Q4_0   ? enqueue_segment_t<CRABML_HIP_Q4_0>(c, seg)
             : c->wtype == CRABML_HIP_Q8_0 ? enqueue_segment_t<CRABML_HIP_Q8_0>(c, seg)
             : c->wtype == CRABML_HIP_Q5_0 ? enqueue_segment_t<CRABML_HIP_Q5_0>(c, seg)
             : c->wtype == CRABML_HIP_Q5_1 ? enqueue_segment_t<CRABML_HIP_Q5_1>(c, seg)
                                           : enqueue_segment_t<CRABML_HIP_Q4_1>(c, seg);
    case SegPath::PerOp:
      break;
  }
  return enqueue_segment_generic(c, seg);
}

TpP2P p2p_view(const crabml_hip_tp_comm* m) {
  TpP2P t{};
  if (m && m->p2p) {
    for (int i = 0; i < 8; i++) t.peer[i] = (unsigned long long*)m->peer[i];
    t.n = m->nranks;
    t.me = m->rank;
    t.cap = m->cap;
    t.fault = m->fault;
  }
  return t;
}

int allreduce(crabml_hip_llama* c, int seg) {
  crabml_hip_device* dev = c->dev;
  if (c->tp_dry) return 0;  // timing-only rank: the partial sums are left as they are
  if (c->comm && c->comm->p2p) {  // one-shot P2P all-reduce as its own launch (per-op segment path)
    if (c->plan.norm_epi) return 0;    // fast path: the collective is fused into the wo / ffn_down epilogue
    const int n = (int)c->cfg.embedding_dim;
    k_tp_allreduce<<<(n + 255) / 256, 256, 0, dev->stream>>>(c->partial, n, tp_view(c, true), c->state + 4, n_segments(c), seg, 0u, 0);
    CH_HIP(dev, hipGetLastError());
    return 0;
  }
  Rccl* r = rccl();
  if (!r || !c->comm || !c->comm->nccl) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama tp: no RCCL communicator");
  int rc = r->AllReduce(c->partial, c->partial, c->cfg.embedding_dim, /*ncclFloat32*/ 7, /*ncclSum*/ 0, c->comm->nccl, dev->stream);
  if (rc != 0) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "ncclAllReduce failed: %s", r->GetErrorString ? r->GetErrorString(rc) : "?");
  return 0;
}

int enqueue_step(crabml_hip_llama* c) {
  const int n = n_segments(c);
  for (int s = 0; s < n; s++) {
    CH_TRY(enqueue_segment(c, s));
    if (c->tp > 1 && s + 1 < n) CH_TRY(allreduce(c, s));
  }
  return 0;
}

// One decode step with attention variant `variant`, captured into a graph and instantiated (llama_create_impl: the greedy step, per
// variant; run_step_sampled: the step that ends in the sampler, c->sampling set around the call).  False: nothing is left behind, and
// the caller decides what that means.  begin_error (optional): what hipStreamBeginCapture answered.
bool capture_step(crabml_hip_llama* c, int variant, hipGraph_t* graph_out, hipGraphExec_t* exec_out, hipError_t* begin_error = nullptr) {
  hipStream_t st = c->dev->stream;
  const hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (begin_error) *begin_error = e;
  if (e != hipSuccess) return false;
  c->capturing = true;
  c->attn_variant = variant;
  const int erc = enqueue_step(c);
  c->capturing = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  const hipError_t e2 = hipStreamEndCapture(st, &graph);
  if (erc == 0 && e2 == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
    *graph_out = graph;
    *exec_out = exec;
    return true;
  }
  if (graph) (void)hipGraphDestroy(graph);
  return false;
}

// one decode step at cache position `pos` (the host tracks it; the kernels read their own copy from device memory)
int run_step(crabml_hip_llama* c, size_t pos) {
  const int variant = variant_of(c, pos);
  if (c->use_graph && c->exec[variant]) {
    CH_HIP(c->dev, hipGraphLaunch(c->exec[variant], c->dev->stream));
    return 0;
  }
  c->attn_variant = variant;
  return enqueue_step(c);
}

// the same step ending in the temperature / top-p sampler: its own graphs (captured on first use, so the greedy ones stay as
// they are), eager under CRABML_HIP_LLAMA_NO_GRAPH
int run_step_sampled(crabml_hip_llama* c, size_t pos) {
  const int variant = variant_of(c, pos);
  crabml_hip_device* dev = c->dev;
  int rc = 0;
  c->sampling = true;
  if (c->use_graph && !c->sexec[variant]) {
    hipError_t begin = hipSuccess;
    if (!capture_step(c, variant, &c->sgraph[variant], &c->sexec[variant], &begin)) {
      c->sampling = false;
      if (begin != hipSuccess) return hip_fail(dev, begin, "llama: sampler graph capture", __FILE__, __LINE__);
      (void)hipGetLastError();
      CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: hipGraph capture/instantiate of the sampled step failed");
    }
  }
  if (c->use_graph) {
    const hipError_t e = hipGraphLaunch(c->sexec[variant], dev->stream);
    if (e != hipSuccess) rc = hip_fail(dev, e, "hipGraphLaunch (sampled step)", __FILE__, __LINE__);
  } else {
    c->attn_variant = variant;
    rc = enqueue_step(c);
  }
  c->sampling = false;
  return rc;
}

// `slots` consecutive 4-int slots of the context's pinned ring.  Past the end every slot may still be waiting for its copy: drain the
// stream, start over.
int next_state_slot(crabml_hip_llama* c, unsigned slots, int** out) {
  if (c->h_state_next + slots > crabml_hip_llama::H_STATE_SLOTS) {
    CH_HIP(c->dev, hipStreamSynchronize(c->dev->stream));
    c->h_state_next = 0;
  }
  *out = c->h_state + 4 * c->h_state_next;
  c->h_state_next += slots;
  return 0;
}

// a few bytes host -> device in stream order, staged through the context's pinned ring (see set_state)
int stage_h2d(crabml_hip_llama* c, void* dst, const void* src, size_t bytes) {
  int* st = nullptr;
  CH_TRY(next_state_slot(c, 1, &st));
  memcpy(st, src, bytes < 16 ? bytes : 16);
  CH_HIP(c->dev, hipMemcpyAsync(dst, st, bytes < 16 ? bytes : 16, hipMemcpyHostToDevice, c->dev->stream));
  return 0;
}

int sample_alloc(crabml_hip_llama* c) {
  if (c->sm_hist) return 0;
  const size_t n = c->cfg.vocab_size;
  CH_TRY(dalloc(c, SAMPLE_BLOCKS * 4, (void**)&c->sm_bmax));
  CH_TRY(dalloc(c, (n * 2 + 15) / 16 * 16, (void**)&c->sm_keys));
  CH_TRY(dalloc(c, 16, (void**)&c->sm_par));
  CH_TRY(dalloc(c, (size_t)c->out_cap * 4, (void**)&c->sm_coins));
  void* h = nullptr;
  CH_TRY(dalloc(c, SAMPLE_HIST * 4, &h));
  CH_HIP(c->dev, hipMemsetAsync(h, 0, SAMPLE_HIST * 4, c->dev->stream));
  c->sm_hist = (unsigned*)h;
  return 0;
}

// the sampler's arguments (sampler.rs:28-52) that the reference panics on or mishandles are refused
bool sample_args_ok(float temperature, float topp) { return temperature >= 0.f && topp > 0.f && !std::isnan(topp); }


// ---- batched prefill ---------------------------------------------------------------------------------------
// B prompt rows at positions pos0 .. pos0 + B - 1 through every layer as (B, k) matmul_vec calls (launch_gemv: MFMA
// GEMM for Q4_0 / Q8_0 and B >= 16), row-wise rmsnorm / quantize / rope / append, and causal attention (row r sees
// pos0 + r + 1 cached positions).  Per row this is the arithmetic of the per-op segment path.
int prefill_alloc(crabml_hip_llama* c, size_t cap) {
  if (c->pf_cap >= cap) return 0;
  if (c->pf_cap != 0) CH_BAIL(c->dev, CRABML_HIP_UNEXPECTED, "llama prefill: row buffers already sized for %zu rows", c->pf_cap);
  const auto& g = c->cfg;
  const size_t dim = g.embedding_dim, kv_dim = (size_t)c->kv_dim_l, hidden = g.hidden_dim;
  auto A = [&](size_t bytes, void** out) { return dalloc(c, bytes ? bytes : 16, out); };
  auto act_bytes = [](uint32_t t, size_t n) { return t == CRABML_HIP_F32 ? (size_t)16 : act_layout(t, n).total; };
  CH_TRY(A(cap * 4, (void**)&c->pf_tokens));
  CH_TRY(A(cap * dim * 4, (void**)&c->pf_x));
  CH_TRY(A(cap * dim * 4, (void**)&c->pf_xn));
  CH_TRY(A(cap * dim * 4, (void**)&c->pf_q));
  CH_TRY(A(cap * kv_dim * 4, (void**)&c->pf_k));
  CH_TRY(A(cap * kv_dim * 4, (void**)&c->pf_v));
  CH_TRY(A(cap * dim * 4, (void**)&c->pf_qr));
  CH_TRY(A(cap * dim * 4, (void**)&c->pf_attn));
  CH_TRY(A(cap * dim * 4, (void**)&c->pf_tmp));
  CH_TRY(A(cap * hidden * 4, (void**)&c->pf_g));
  CH_TRY(A(cap * hidden * 4, (void**)&c->pf_u));
  CH_TRY(A(cap * act_bytes(c->qt, dim), (void**)&c->pf_act_dim));
  CH_TRY(A(cap * act_bytes(c->qt, hidden), (void**)&c->pf_act_hid));
  if ((c->qt == CRABML_HIP_Q8_0 || c->qt == CRABML_HIP_Q8_1 || c->qt == CRABML_HIP_Q8_K) && !c->dev->strict_order) {  // (whole column tiles + the look-ahead's slack)
    const size_t xb = gemm_f16w_xh_bytes(cap, dim > hidden ? dim : hidden);
    CH_TRY(A(xb, &c->pf_xh));
    CH_TRY(A(xb, &c->pf_xh2));
    CH_HIP(c->dev, hipMemsetAsync(c->pf_xh2, 0, xb, c->dev->stream));
    // (the widest split launch is q | k | v; up to 7 partial buffers of a short pass, 3 of a full one)
    c->pf_split_floats = (cap + 1024) * (dim + 2 * kv_dim > hidden ? dim + 2 * kv_dim : hidden);
    CH_TRY(A(c->pf_split_floats * 4, (void**)&c->pf_split));
    CH_HIP(c->dev, hipMemsetAsync(c->pf_xh, 0, xb, c->dev->stream));
    CH_TRY(A(16, (void**)&c->pf_ovf));
    CH_HIP(c->dev, hipMemsetAsync(c->pf_ovf, 0, 16, c->dev->stream));
  }
  c->pf_cap = cap;
  return 0;
}


// The prompt pass's exact kernels (k_attn_tile, the long-rows kernels) exist for these GQA groups, and NO_TILE_ATTENTION switches both
// off.  The launch sites dispatch through this list and create's long_cache_refusal asks it: one list, one flag test.
template <class F>
bool with_exact_rows_group(int grp, F&& f) { return with_const<1, 2, 4, 8>(grp, f); }
bool exact_rows_group(int grp) { return with_exact_rows_group(grp, [](auto) {}); }
bool exact_rows_on(const crabml_hip_llama_config_t& g) { return !(g.flags & CRABML_HIP_LLAMA_NO_TILE_ATTENTION); }

// the row-tiled causal attention of a prefill pass; false = not covered (the caller launches k_attn per (head, row))
template <bool KV16, int G, int R>
bool launch_attn_tile_t(crabml_hip_llama* c, int l, int B, int pos0) {
  const int hd = c->hd, n_heads = c->n_heads_l, n_kv = c->n_kv_l, seq_cap = (int)c->cfg.seq_len;
  const int sstride = (pos0 + B + 3) & ~3;
  const size_t lds = (size_t)(G * R) * (size_t)(hd + sstride) * sizeof(float);
  if (lds > 64 * 1024) return false;
  k_attn_tile<KV16, G, R><<<dim3(n_kv, (B + R - 1) / R), 256, lds, c->dev->stream>>>(
      c->pf_qr, c->kc[l], c->vc[l], c->state + 6, (const unsigned short*)c->dev->exp_table, c->pf_attn, n_heads, n_kv, hd, seq_cap, B,
      sstride);
  return true;
}
bool launch_attn_tile(crabml_hip_llama* c, int l, int B, int pos0) {
  const int hd = c->hd, g = c->n_heads_l / c->n_kv_l;
  const bool kv16 = c->cfg.use_f16_kv_cache != 0;
  if (!exact_rows_on(c->cfg)) return false;
  if (pos0 + B > 1024 || hd > (kv16 ? 256 : 128) || hd % (kv16 ? 16 : 4) != 0 || c->n_heads_l % c->n_kv_l != 0) return false;
  bool ok = false;  // (other group sizes: not covered)
  with_const_else<0, 1>(kv16, [&](auto kv) {
    with_exact_rows_group(g, [&](auto grp) {
      constexpr int G = decltype(grp)::value;
      ok = launch_attn_tile_t<decltype(kv)::value != 0, G, (G == 8 ? 2 : 4)>(c, l, B, pos0);  // rows per workgroup: G = 8 fills the lanes with two
    });
  });
  return ok;
}

// prompts past 1024 positions: the three long-context kernels with a row dimension (grid.y), PF_LONG_ROWS rows at a time
// (score / probability scratch: rows x n_heads x seq_len x 6 bytes)
constexpr int PF_LONG_ROWS = 64;
template <int G>
int launch_attn_long_rows_t(crabml_hip_llama* c, int l, int B) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const int hd = c->hd, seq_cap = (int)c->cfg.seq_len, n_kv = c->n_kv_l, n_heads = c->n_heads_l;
  const int* pos_d = c->state + 6;
  const int ts = 256 / G, nsplit = (seq_cap + ts - 1) / ts;
  if (!c->pf_scores) {
    CH_TRY(dalloc(c, (size_t)PF_LONG_ROWS * n_heads * seq_cap * 4, (void**)&c->pf_scores));
    CH_TRY(dalloc(c, (size_t)PF_LONG_ROWS * n_heads * seq_cap * 2, (void**)&c->pf_p16));
  }
  for (int r0 = 0; r0 < B; r0 += PF_LONG_ROWS) {
    const unsigned rows = (unsigned)(B - r0 < PF_LONG_ROWS ? B - r0 : PF_LONG_ROWS);
    k_attn_scores<G><<<dim3(n_kv * nsplit, rows), 256, (size_t)G * hd * sizeof(float), st>>>(
        (const float*)c->pf_qr, (const unsigned short*)c->kc[l], pos_d, c->pf_scores, n_kv, hd, seq_cap, nsplit, r0);
    k_attn_softmax<4><<<dim3(n_heads, rows), 256, (size_t)seq_cap * sizeof(float), st>>>(
        (const float*)c->pf_scores, pos_d, (const unsigned short*)dev->exp_table, c->pf_p16, seq_cap, r0, dev->strict_order ? 1 : 0);
    // PV for R prompt rows per workgroup (one V fetch for R x G chains); G = 8 fills the lanes with two rows
    constexpr int PR = G == 8 ? 2 : 4;
    if (c->cfg.flags & CRABML_HIP_LLAMA_NO_PV_ROW_TILES)
      k_attn_pv<G><<<dim3(n_kv * (hd / 32), rows), 256, 0, st>>>((const unsigned short*)c->pf_p16, (const unsigned short*)c->vc[l], pos_d,
                                                                 c->pf_attn, nullptr, nullptr, nullptr, hd, seq_cap, 0, r0);
    else
      k_attn_pv_rows<G, PR><<<dim3(n_kv * (hd / 32), (rows + PR - 1) / PR), 256, 0, st>>>(
          (const unsigned short*)c->pf_p16, (const unsigned short*)c->vc[l], pos_d, c->pf_attn, hd, seq_cap, r0, (int)rows);
  }
  return 0;
}
// 1 = launched, 0 = not covered, < 0 = error
int launch_attn_long_rows(crabml_hip_llama* c, int l, int B) {
  if (!c->plan.exact_long_ok || !exact_rows_on(c->cfg)) return 0;
  int rc = 0;
  if (!with_exact_rows_group(c->n_heads_l / c->n_kv_l, [&](auto grp) { rc = launch_attn_long_rows_t<decltype(grp)::value>(c, l, B); })) return 0;
  return rc == 0 ? 1 : -1;
}

// The causal attention of a prompt pass for layer l (pf_qr x KV cache -> pf_attn): the one place that chooses among the four forms.
// Returns the kernel as CRABML_HIP_PFPLAN_ATTN_KERNEL names it (1 flash rows, 2 tile, 3 long rows, 4 per (head, row)), < 0 = error.
int launch_prefill_attention(crabml_hip_llama* c, int l, size_t B, size_t pos0) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const int hd = c->hd, n_heads = c->n_heads_l, n_kv = c->n_kv_l, seq_cap = (int)c->cfg.seq_len;
  const bool kv16 = c->cfg.use_f16_kv_cache != 0;
  const int* pos_d = c->state + 6;
  // (a pass whose every row sees fewer cached positions than the decode step's switch to the f32 kernels -- attn_long_from --
  // keeps the exact tile kernel, so that prefill(prompt) and a token loop over the same short prompt agree bit for bit)
  if (c->plan.attn_flash_rows && kv16 && pos0 + B >= c->plan.attn_long_from) {
    // fast step: causal flash attention on the f16 matrix cores (k_attn_flash_rows; the deviation stated for k_attn_flash)
    const dim3 fg((unsigned)((B + 63) / 64), (unsigned)n_heads);
    flash_rows_kernel(hd)<<<fg, 512, flash_rows_lds_bytes(hd), st>>>((const float*)c->pf_qr, (const unsigned short*)c->kc[l],
                                                                      (const unsigned short*)c->vc[l], pos_d, c->pf_attn, n_heads, n_kv, seq_cap, (int)B);
    return 1;
  }
  if (launch_attn_tile(c, l, (int)B, (int)pos0)) return 2;
  const int along = launch_attn_long_rows(c, l, (int)B);  // past 1024 positions: the long-context kernels, rows in grid.y
  if (along != 0) return along < 0 ? -1 : 3;
  // unusual shapes (f32 cache past 1024 positions, odd group sizes): one workgroup per (head, row), its score row sized by the positions
  // the pass's last row sees (rounded as k_attn_tile's sstride, never past the cache), not by the cache
  const int row_cap = std::min((int)((pos0 + B + 3) & ~(size_t)3), seq_cap);
  const size_t attn_lds = k_attn_lds_bytes(row_cap, hd);
  if (attn_lds > K_ATTN_LDS) {
    (void)set_error(dev, CRABML_HIP_UNEXPECTED, "llama prefill: no attention kernel of this context takes a pass that sees %zu positions",
                    pos0 + B);
    return -1;
  }
  with_const_else<0, 1>(kv16, [&](auto kv) {
    k_attn<decltype(kv)::value != 0><<<dim3(n_heads, (unsigned)B), 256, attn_lds, st>>>(c->pf_qr, c->kc[l], c->vc[l], pos_d,
                                                                                        (const unsigned short*)dev->exp_table, c->pf_attn, nullptr, nullptr,
                                                                                        nullptr, n_heads, n_kv, hd, seq_cap, row_cap, PrefetchPlan{},
                                                                                        dev->strict_order ? 256 : 0);
  });
  return 4;
}

// What c->pf_xh holds: the planes it mirrors as pre-scaled f16 (null = nothing usable) and the k-slot order it is in
// (gemm_f16w_order of the weight format that reads it)
struct XhHolds {
  const void* planes = nullptr;
  int order = -1;
  bool holds(const void* p, int o) const { return planes == p && order == o; }
  void set(const void* p, int o) {
    planes = p;
    order = o;
  }
  // ffn_down's planes were written to pf_xh2 while pf_xh was the gate | up launch's own rhs: ffn_down's GEMM reads what that launch wrote
  static void swap(crabml_hip_llama* c) { std::swap(c->pf_xh, c->pf_xh2); }
};

// allow_f16w = false: the pass keeps the int8 GEMMs (prefill_chunk's recomputation of a chunk whose B' overflowed f16)
int prefill_chunk_pass(crabml_hip_llama* c, const uint32_t* tokens, size_t B, size_t pos0, bool want_logits, bool allow_f16w, bool* f16w_used) {
  crabml_hip_device* dev = c->dev;
  hipStream_t st = dev->stream;
  const auto& g = c->cfg;
  const int dim = (int)g.embedding_dim, kv_dim = c->kv_dim_l, hidden = (int)g.hidden_dim, hd = c->hd, seq_cap = (int)g.seq_len;
  const int L = (int)g.n_layers;
  const bool kv16 = g.use_f16_kv_cache != 0, strict = dev->strict_order;
  const int half = strict ? 0 : 1;
  const unsigned rows = (unsigned)B;
  {
    std::vector<int> h(B + 1);
    for (size_t i = 0; i < B; i++) h[i] = (int)tokens[i];
    CH_HIP(dev, hipMemcpyAsync(c->pf_tokens, h.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
    const int p0 = (int)pos0;
    CH_HIP(dev, hipMemcpyAsync(c->state + 6, &p0, sizeof(int), hipMemcpyHostToDevice, st));
    CH_HIP(dev, hipStreamSynchronize(st));  // the staging vectors go out of scope
  }
  const int* pos_d = c->state + 6;
  const size_t norm_lds = norm_lds_bytes(dim);
  auto norm_rows = [&](const float* wn, float eps) {
    with_const_else<4, 12>(norm_nit(dim), [&](auto nit) {
      k_norm_f32_rows<decltype(nit)::value><<<rows, 1024, norm_lds, st>>>(c->pf_x, wn, dim, eps, c->pf_xn, half);
    });
  };
  // A/B hook (CRABML_HIP_TEST_HOOKS=1 CRABML_HIP_GEMM_EXACT=1): the fast pass with matmul_vec's own scaling
  static const bool gemm_exact_hook = test_hook_on("CRABML_HIP_GEMM_EXACT");
  // The fast pass, Q4_0 / Q8_0 / Q5_0 weights x Q8_0 rows, Q4_1 / Q5_1 x Q8_1, Q4_K / Q6_K / Q2_K / Q3_K (Q5_K: opt-in) x Q8_K, >= 32 rows: the weight-stationary f16 GEMM
  // (gemm_f16w.hip; block scales folded into f16 operands, f32 accumulation inside the matrix core -- a stated deviation of the fast
  // tier).  The rows' pre-scaled f16 planes are made once per rhs and k-slot order (q / k / v and gate / up share theirs): `xh`
  // remembers what pf_xh currently holds.
  // A/B hook (CRABML_HIP_TEST_HOOKS=1 CRABML_HIP_GEMM_INT8=1): the int8 kernels in the fast pass too
  static const bool f16w_off = test_hook_on("CRABML_HIP_GEMM_INT8");
  // lab hook (CRABML_HIP_TEST_HOOKS=1 CRABML_HIP_F16W_MIN=rows): the smallest pass that takes it
  static const int f16w_min = test_hook_int("CRABML_HIP_F16W_MIN", 32);
  const bool f16w = allow_f16w && !strict && !gemm_exact_hook && !f16w_off && !(g.flags & CRABML_HIP_LLAMA_PREFILL_INT8_GEMM) &&
                    (c->qt == CRABML_HIP_Q8_0 || c->qt == CRABML_HIP_Q8_1 || c->qt == CRABML_HIP_Q8_K) && c->pf_xh != nullptr && B >= f16w_min;  // (shorter passes: the int8 kernels / the GEMV)
  *f16w_used = f16w;
  int* const ovf = c->pf_ovf;
  // the f16 GEMM takes matrix w, whose rows are k elements long (Q8_K rows: whole super-blocks only).  The one predicate: the GEMMs,
  // the kernels that write pf_xh ahead of them and the two one-launch sites all ask here.
  // (a Q5_K matrix: only in a context created with CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM on one device -- without it Q5_K keeps the row GEMV
  // in every body, as the launch pins of the K-quant passes state)
  auto takes_f16w = [&](const crabml_hip_buf* w, int k) {
    if (w->dtype == CRABML_HIP_Q5_K && !((g.flags & CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM) && c->tp == 1)) return false;
    return f16w && gemm_f16w_takes(dev, w, c->qt) && (c->qt != CRABML_HIP_Q8_K || k % 256 == 0);
  };
  XhHolds xh;
  auto rows_to_f16 = [&](const crabml_hip_buf* w, const void* act, int k) -> bool {  // true: pf_xh was made here
    const int order = gemm_f16w_order(w->dtype);
    if (xh.holds(act, order)) return false;
    launch_rows_to_f16(st, c->qt, w->dtype, act, B, (size_t)k, c->pf_xh, ovf);
    xh.set(act, order);
    return true;
  };
  // ... written by the kernel that quantizes the rows when the GEMM that reads them next is the f16 one (f16w_rows.hpp: the same
  // bits as k_rows_to_f16 from the finished planes, one launch fewer per GEMM; A/B: CRABML_HIP_LLAMA_PREFILL_SEPARATE_F16_ROWS)
  auto xh_target = [&](const crabml_hip_buf* next, int k, int* order) -> void* {
    if (next == nullptr || (g.flags & CRABML_HIP_LLAMA_PREFILL_SEPARATE_F16_ROWS) || !takes_f16w(next, k)) return nullptr;
    *order = gemm_f16w_order(next->dtype);
    return c->pf_xh;
  };
  // CpuTensorBuf::quantize for the rhs of matmul_vec (buf/api.rs:142-159): F32 weights take the rows as they are
  // next: the weight matrix whose GEMM reads these planes first
  auto quant_rows = [&](const float* src, int n, char* planes, const crabml_hip_buf* next) -> const void* {
    if (c->qt == CRABML_HIP_F32) return src;
    int order = 0;
    void* mirror = xh_target(next, n, &order);
    launch_quantize_act_rows(st, c->qt, src, B, (size_t)n, planes, mirror, order, ovf);
    xh.set(mirror ? planes : nullptr, order);
    return planes;
  };
  // defer (nullable): a GEMM cut into k pieces may leave the sum of its pieces to the row kernel that consumes `out` (pf_split holds them)
  // fc / xh_field / kword (prefill tap only): the launch form as taken, the tap field B' goes to as this GEMM finds it (xh_if_made: only
  // where this GEMM had to re-make pf_xh), and the plan word that says which kernel the matrix took (CRABML_HIP_PFPLAN_KERNEL_*)
  TapRec& tap = c->pftap;
  auto gemm = [&](const crabml_hip_buf* w, int m, int k, const void* act, float* out, int* defer = nullptr, F16wForce* fc = nullptr,
                  int xh_field = -1, int kword = -1, bool xh_if_made = false) -> int {
    auto took = [&](int kernel) {
      if (kword >= 0) tap.note(kword, kernel);
    };
    if (defer) *defer = 0;
    if (g.flags & CRABML_HIP_LLAMA_PREFILL_SEPARATE_F16_ROWS) defer = nullptr;  // (A/B: every reduce its own launch)
    if (takes_f16w(w, k)) {
      const bool made = rows_to_f16(w, act, k);
      if (xh_field >= 0 && (made || !xh_if_made)) CH_TRY(tap.copy(c, xh_field, c->pf_xh, B * (size_t)k * 2));
      const size_t mm = (size_t)m;
      if (launch_gemm_f16w(dev, &w, &mm, 1, (size_t)k, c->pf_xh, B, &out, c->pf_split, c->pf_split_floats, nullptr, nullptr, defer, nullptr, fc)) {
        took(1);
        return 0;
      }
    }
    if (!strict) {
      if (kword >= 0 && tap.armed()) {  // launch_gemv's own first question, asked here so that the plan can say what it answered
        if (B >= 16 && launch_gemm_mfma(dev, w, m, k, act, B, out, nullptr, nullptr, !gemm_exact_hook)) {
          took(2);
          return 0;
        }
        took(3);
      }
      return launch_gemv(dev, w, m, k, act, B, out, nullptr, !gemm_exact_hook);
    }
    // strict order: the Q4_0 / Q8_0 / Q4_1 MFMA GEMM scales its exact integer tiles block by block in the reference's scalar
    // order, i.e. it IS the strict result (bit for bit) -- the other formats take the scalar-order GEMV row by row
    if ((w->dtype == CRABML_HIP_Q4_0 || w->dtype == CRABML_HIP_Q8_0 || w->dtype == CRABML_HIP_Q4_1 || w->dtype == CRABML_HIP_Q8_K) && B >= 16 &&
        launch_gemm_mfma(dev, w, m, k, act, B, out, nullptr))
      return 0;
    return launch_gemv_strict(dev, w, m, k, act, B, out);
  };
  k_embed<<<dim3((dim + 255) / 256, rows), 256, 0, st>>>((const char*)c->token_embed->ptr, (int)c->token_embed->dtype,
                                                         c->token_embed->wl.off_scale, c->pf_tokens, dim, c->pf_x, c->embed_scale);
  // Q8_0 / Q8_1 rhs: residual add + RMSNorm + quantize as one launch per row (k_norm_quant_rows), SiLU * mul + quantize as one
  // (k_gateup_epi_quant): the (rows, dim) / (rows, hidden) f32 intermediates make one trip through memory instead of three
  const bool fuse_rows = (c->qt == CRABML_HIP_Q8_0 || c->qt == CRABML_HIP_Q8_1) && !(g.flags & CRABML_HIP_LLAMA_NO_PREFILL_ROW_FUSION);
  // Q8_K rhs (K-quant layers): the same for residual add + RMSNorm + quantize (k_norm_quant_rows_k); SiLU * mul keeps its own launch
  // (from 192 rows: one 1024-thread workgroup per row is a chain of four barriers -- below, the four small launches run 1-2 % faster)
  const bool fuse_k = c->qt == CRABML_HIP_Q8_K && dim % 256 == 0 && B >= 192 && !(g.flags & CRABML_HIP_LLAMA_NO_PREFILL_ROW_FUSION);
  const bool fuse_norm = fuse_rows || fuse_k;
  const ActLayout ald = act_layout(c->qt == CRABML_HIP_F32 ? CRABML_HIP_Q8_0 : c->qt, (size_t)dim);
  const ActLayout alh = act_layout(c->qt == CRABML_HIP_F32 ? CRABML_HIP_Q8_0 : c->qt, (size_t)hidden);
  // pending = the wo / ffn_down output that has not been added to x yet (folded into the next norm)
  // nparts: `pending` is piece 0 of a GEMM cut into k pieces, the others wait in pf_split (gemm's defer)
  int norm_kernel = 0;  // (prefill tap: which of them the last call launched -- CRABML_HIP_PFPLAN_NORM_KERNEL, read after the first norm)
  auto norm_quant_rows = [&](const float* wn, float eps, float* pending, const crabml_hip_buf* next, int nparts = 0) -> const void* {
    const bool q81 = c->qt == CRABML_HIP_Q8_1;
    int order = 0;
    unsigned short* mirror = (unsigned short*)xh_target(next, dim, &order);
    const size_t pstride = B * (size_t)dim;
    // Q8_0 / Q8_1 rows of 4096 / 8192 elements: the 256-thread form (a thread owns half a quant block / a whole one; prefill_rows.hpp)
    // lab hook (CRABML_HIP_TEST_HOOKS=1 CRABML_HIP_NORM_ROWS_1024=1): the 1024-thread kernel
    static const bool rows_1024 = test_hook_on("CRABML_HIP_NORM_ROWS_1024");
    if (!fuse_k && !rows_1024 && (dim == 4096 || dim == 8192) && !(g.flags & CRABML_HIP_LLAMA_PREFILL_SEPARATE_F16_ROWS)) {
      norm_kernel = 3;
      with_const_else<16, 32>(dim / 256, [&](auto ec) {  // elements per thread
        with_const_else<0, 1>(q81, [&](auto q) {
          k_norm_quant_rows_w<decltype(ec)::value, decltype(q)::value != 0><<<rows, 256, 0, st>>>(
              c->pf_x, pending, wn, dim, eps, c->pf_act_dim, ald.total, ald.off_d, ald.off_aux, half, mirror, c->pf_split, pstride, nparts, ovf);
        });
      });
    } else if (fuse_k) {
      norm_kernel = 4;
      with_const_else<4, 12>(norm_nit(dim), [&](auto nit) {
        k_norm_quant_rows_k<decltype(nit)::value><<<rows, 1024, norm_lds, st>>>(c->pf_x, pending, wn, dim, eps, c->pf_xn, c->pf_act_dim, ald.total,
                                                                                ald.off_d, ald.off_aux, ald.off_p, half, mirror, order, c->pf_split,
                                                                                pstride, nparts, ovf);
      });
    } else {
      with_const_else<4, 12>(norm_nit(dim), [&](auto nit) {
        with_const_else<0, 1>(q81, [&](auto q) {
          constexpr int NIT = decltype(nit)::value;
          constexpr bool Q = decltype(q)::value != 0;
          if (mirror || nparts > 0) {  // (f16 planes alongside, or pieces of a cut GEMM to add first: prefill_rows.hpp)
            norm_kernel = 2;
            k_norm_quant_rows_h<NIT, Q><<<rows, 1024, norm_lds, st>>>(c->pf_x, pending, wn, dim, eps, c->pf_act_dim, ald.total, ald.off_d, ald.off_aux,
                                                                      half, mirror, c->pf_split, pstride, nparts, ovf);
          } else {
            norm_kernel = 1;
            k_norm_quant_rows<NIT, Q><<<rows, 1024, norm_lds, st>>>(c->pf_x, pending, wn, dim, eps, c->pf_act_dim, ald.total, ald.off_d, ald.off_aux,
                                                                    half);
          }
        });
      });
    }
    xh.set(mirror ? c->pf_act_dim : nullptr, order);
    return c->pf_act_dim;
  };
  bool pending_down = false;  // (fuse_rows) the previous layer's ffn_down output sits in pf_tmp, not yet added to pf_x
  int down_parts = 0;         // ... as piece 0 of this many + 1 k pieces
  // the prefill tap (test hook): host-side copies between the launches of the tapped layer, the launch plan noted where it is decided;
  // no-ops unless a tapped pass is being enqueued
  const size_t xb_dim = B * (size_t)dim * 4, xb_kv = B * (size_t)kv_dim * 4, xb_hid = B * (size_t)hidden * 4;
  auto PT = [&](bool on, int f, const void* src, size_t bytes) -> int { return on ? tap.copy(c, f, src, bytes) : 0; };
  auto note_form = [&](int l, int word_f, const F16wForce& fc) {
    tap.note(l, word_f, fc.used_F);
    tap.note(l, word_f + 1, fc.used_T);
    tap.note(l, word_f + 2, fc.used_ksplit);
  };
  tap.note(CRABML_HIP_PFPLAN_F16W, f16w ? 1 : 0);
  for (int l = 0; l < L; l++) {
    const bool tl = tap.layer == l;
    const bool down_deferred = fuse_norm && l + 1 < L;  // ffn_down's add is left to the next layer's norm
    const void* a;
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_IN_X, c->pf_x, xb_dim));
    if (fuse_norm) {
      const int in_parts = pending_down ? down_parts : 0;
      CH_TRY(PT(tl && pending_down, CRABML_HIP_PFTAP_IN_TMP, c->pf_tmp, xb_dim));
      CH_TRY(PT(tl && in_parts > 0, CRABML_HIP_PFTAP_IN_PARTS, c->pf_split, (size_t)in_parts * xb_dim));
      tap.note(l, CRABML_HIP_PFPLAN_IN_PARTS, in_parts);
      a = norm_quant_rows((const float*)c->rms_att[l]->ptr, g.rms_norm_eps, pending_down ? c->pf_tmp : nullptr, c->wq[l], in_parts);
      pending_down = false;
    } else {
      norm_rows((const float*)c->rms_att[l]->ptr, g.rms_norm_eps);  // llama2.rs:230-234
      a = quant_rows(c->pf_xn, dim, c->pf_act_dim, c->wq[l]);
    }
    tap.note(l, CRABML_HIP_PFPLAN_NORM_KERNEL, fuse_norm ? norm_kernel : 0);
    const bool xn_stored = !fuse_norm || fuse_k;  // (k_norm_f32_rows and k_norm_quant_rows_k leave the f32 norm in pf_xn)
    CH_TRY(PT(tl && xn_stored, CRABML_HIP_PFTAP_N1_XN, c->pf_xn, xb_dim));
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_N1_X, c->pf_x, xb_dim));
    CH_TRY(PT(tl && c->qt != CRABML_HIP_F32, CRABML_HIP_PFTAP_N1_ACT, c->pf_act_dim, B * ald.total));
    F16wForce fc_qkv{}, fc_wo{}, fc_gu{}, fc_down{};  // (all zero: the launcher's own choice; read back for the plan)
    bool qkv_done = false;  // llama2.rs:244-246
    if (takes_f16w(c->wq[l], dim) && c->wk[l]->dtype == c->wq[l]->dtype && c->wv[l]->dtype == c->wq[l]->dtype) {
      // the three GEMMs of the same rhs as ONE launch (the 1024-row k / v matrices alone leave most of the chip idle)
      rows_to_f16(c->wq[l], a, dim);
      CH_TRY(PT(tl, CRABML_HIP_PFTAP_N1_XH, c->pf_xh, B * (size_t)dim * 2));
      const crabml_hip_buf* ws[3] = {c->wq[l], c->wk[l], c->wv[l]};
      const size_t ms[3] = {(size_t)dim, (size_t)kv_dim, (size_t)kv_dim};
      float* outs[3] = {c->pf_q, c->pf_k, c->pf_v};
      qkv_done = launch_gemm_f16w(dev, ws, ms, 3, (size_t)dim, c->pf_xh, B, outs, c->pf_split, c->pf_split_floats, nullptr, nullptr, nullptr,
                                  nullptr, tl ? &fc_qkv : nullptr);
      if (qkv_done)
        for (int kw : {CRABML_HIP_PFPLAN_KERNEL_Q, CRABML_HIP_PFPLAN_KERNEL_K, CRABML_HIP_PFPLAN_KERNEL_V}) tap.note(l, kw, 1);
    }
    if (!qkv_done) {
      CH_TRY(gemm(c->wq[l], dim, dim, a, c->pf_q, nullptr, tl ? &fc_qkv : nullptr, tl ? CRABML_HIP_PFTAP_N1_XH : -1,
                  tl ? CRABML_HIP_PFPLAN_KERNEL_Q : -1));
      CH_TRY(gemm(c->wk[l], kv_dim, dim, a, c->pf_k, nullptr, nullptr, -1, tl ? CRABML_HIP_PFPLAN_KERNEL_K : -1));
      CH_TRY(gemm(c->wv[l], kv_dim, dim, a, c->pf_v, nullptr, nullptr, tl ? CRABML_HIP_PFTAP_N1_XH_V : -1,
                  tl ? CRABML_HIP_PFPLAN_KERNEL_V : -1, true));
    }
    tap.note(l, CRABML_HIP_PFPLAN_QKV_ONE, qkv_done ? 1 : 0);
    note_form(l, CRABML_HIP_PFPLAN_QKV_F, fc_qkv);
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_Q, c->pf_q, xb_dim));
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_K, c->pf_k, xb_kv));
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_V, c->pf_v, xb_kv));
    QkvEpi e{c->pf_qr, c->kc[l], c->vc[l], c->rope, pos_d, 1.0f / std::sqrt((float)hd), dim, kv_dim, hd,
             (int)g.rope_dim, c->npairs, seq_cap, kv16 ? 1 : 0};
    const int pairs = (dim + 2 * kv_dim) / 2;
    with_qkv_epi(c, e, l, [&](auto ep) {
      k_qkv_epi_rows<QkvArchOf<decltype(ep)>::value><<<dim3((pairs + 255) / 256, rows), 256, 0, st>>>(c->pf_q, c->pf_k, c->pf_v, ep);
    });
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_QR, c->pf_qr, xb_dim));
    const int attn_kernel = launch_prefill_attention(c, l, B, pos0);  // llama2.rs:571-590
    if (attn_kernel < 0) return CRABML_HIP_UNEXPECTED;
    tap.note(l, CRABML_HIP_PFPLAN_ATTN_KERNEL, attn_kernel);
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_ATTN, c->pf_attn, xb_dim));
    a = quant_rows(c->pf_attn, dim, c->pf_act_dim, c->wo[l]);
    CH_TRY(PT(tl && c->qt != CRABML_HIP_F32, CRABML_HIP_PFTAP_ATTN_ACT, c->pf_act_dim, B * ald.total));
    int wo_parts = 0;
    CH_TRY(gemm(c->wo[l], dim, dim, a, c->pf_tmp, fuse_norm ? &wo_parts : nullptr, tl ? &fc_wo : nullptr,
                tl ? CRABML_HIP_PFTAP_ATTN_XH : -1, tl ? CRABML_HIP_PFPLAN_KERNEL_WO : -1));  // llama2.rs:600
    tap.note(l, CRABML_HIP_PFPLAN_WO_PARTS, wo_parts);
    note_form(l, CRABML_HIP_PFPLAN_WO_F, fc_wo);
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_WO_TMP, c->pf_tmp, xb_dim));
    CH_TRY(PT(tl && wo_parts > 0, CRABML_HIP_PFTAP_WO_PARTS, c->pf_split, (size_t)wo_parts * xb_dim));
    if (fuse_norm) {
      a = norm_quant_rows((const float*)c->rms_ffn[l]->ptr, 1e-5f, c->pf_tmp, c->gate[l], wo_parts);  // x += wo out (:266), FFN norm (:611), quantize
    } else {
      k_res_epi<<<(unsigned)(((size_t)B * dim + 255) / 256), 256, 0, st>>>(c->pf_tmp, c->pf_x, (int)(B * dim), 1);  // :266
      norm_rows((const float*)c->rms_ffn[l]->ptr, 1e-5f);  // llama2.rs:611
      a = quant_rows(c->pf_xn, dim, c->pf_act_dim, c->gate[l]);
    }
    CH_TRY(PT(tl && xn_stored, CRABML_HIP_PFTAP_N2_XN, c->pf_xn, xb_dim));
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_N2_X, c->pf_x, xb_dim));
    CH_TRY(PT(tl && c->qt != CRABML_HIP_F32, CRABML_HIP_PFTAP_N2_ACT, c->pf_act_dim, B * ald.total));
    bool gu_done = false;  // llama2.rs:620-630
    int h_done = 0;        // the launch stored h = silu(g) * u (pf_g) instead of g and u
    if (takes_f16w(c->gate[l], dim) && c->up[l]->dtype == c->gate[l]->dtype) {
      // gate and up as ONE launch: 2 x 448 workgroups fill the last round of the chip better than 448 twice -- and, where 64-row tiles
      // of both cover the chip, with SiLU * mul as the epilogue (a wave holds the same 16 rows of both matrices)
      rows_to_f16(c->gate[l], a, dim);
      CH_TRY(PT(tl, CRABML_HIP_PFTAP_N2_XH, c->pf_xh, B * (size_t)dim * 2));
      const crabml_hip_buf* ws[2] = {c->gate[l], c->up[l]};
      const size_t ms[2] = {(size_t)hidden, (size_t)hidden};
      float* outs[2] = {c->pf_g, c->pf_u};
      const bool epi = !(g.flags & CRABML_HIP_LLAMA_PREFILL_NO_GU_EPILOGUE);
      // ... and, for Q8_0 / Q8_1 rows, with the row quantizer behind it (h leaves as ffn_down's planes; its f16 planes go to pf_xh2:
      // pf_xh is this launch's own rhs)
      F16wHQuant hq{};
      int hq_order = 0;
      if (epi && fuse_rows && !(g.flags & CRABML_HIP_LLAMA_PREFILL_SEPARATE_F16_ROWS)) {
        hq.planes = c->pf_act_hid;
        hq.stride = alh.total;
        hq.off_d = alh.off_d;
        hq.off_aux = alh.off_aux;
        hq.q81 = c->qt == CRABML_HIP_Q8_1;
        hq.xh = xh_target(c->down[l], hidden, &hq_order) ? (unsigned short*)c->pf_xh2 : nullptr;
        hq.ovf = ovf;
      }
      gu_done = launch_gemm_f16w(dev, ws, ms, 2, (size_t)dim, c->pf_xh, B, outs, c->pf_split, c->pf_split_floats,
                                 epi ? &c->ffn_act : nullptr, epi ? &h_done : nullptr, nullptr, &hq,
                                 tl ? &fc_gu : nullptr);
      if (h_done == 2) {
        a = c->pf_act_hid;
        if (hq.xh) XhHolds::swap(c);
        xh.set(hq.xh ? c->pf_act_hid : nullptr, hq_order);
      }
      if (gu_done)
        for (int kw : {CRABML_HIP_PFPLAN_KERNEL_GATE, CRABML_HIP_PFPLAN_KERNEL_UP}) tap.note(l, kw, 1);
    }
    if (!gu_done) {
      CH_TRY(gemm(c->gate[l], hidden, dim, a, c->pf_g, nullptr, tl ? &fc_gu : nullptr, tl ? CRABML_HIP_PFTAP_N2_XH : -1,
                  tl ? CRABML_HIP_PFPLAN_KERNEL_GATE : -1));
      CH_TRY(gemm(c->up[l], hidden, dim, a, c->pf_u, nullptr, nullptr, -1, tl ? CRABML_HIP_PFPLAN_KERNEL_UP : -1));
    }
    tap.note(l, CRABML_HIP_PFPLAN_GU_ONE, gu_done ? 1 : 0);
    tap.note(l, CRABML_HIP_PFPLAN_H_DONE, h_done);
    note_form(l, CRABML_HIP_PFPLAN_GU_F, fc_gu);
    CH_TRY(PT(tl && h_done != 2, CRABML_HIP_PFTAP_G, c->pf_g, xb_hid));
    CH_TRY(PT(tl && h_done == 0, CRABML_HIP_PFTAP_U, c->pf_u, xb_hid));
    if (h_done == 2) {
      // (quantized by the launch itself)
    } else if (h_done) {  // h sits in pf_g: quantize it (the quantizer launch's arithmetic is quant_lane32's, bit for bit)
      a = quant_rows(c->pf_g, hidden, c->pf_act_hid, c->down[l]);
    } else if (fuse_rows) {
      const dim3 gq((unsigned)((hidden + 255) / 256), rows);
      int order = 0;
      unsigned short* mirror = (unsigned short*)xh_target(c->down[l], hidden, &order);
      with_const_else<0, 1>(c->qt == CRABML_HIP_Q8_1, [&](auto q) {
        constexpr bool Q = decltype(q)::value != 0;
        if (mirror)  // (ffn_down's f16 planes alongside)
          k_gateup_epi_quant_h<Q><<<gq, 256, 0, st>>>(c->pf_g, c->pf_u, c->ffn_act, hidden, c->pf_act_hid, alh.total,
                                                      alh.off_d, alh.off_aux, mirror, ovf);
        else
          k_gateup_epi_quant<Q><<<gq, 256, 0, st>>>(c->pf_g, c->pf_u, c->ffn_act, hidden, c->pf_act_hid, alh.total,
                                                    alh.off_d, alh.off_aux);
      });
      xh.set(mirror ? c->pf_act_hid : nullptr, order);
      a = c->pf_act_hid;
    } else {
      k_gateup_epi<<<(unsigned)(((size_t)B * hidden + 255) / 256), 256, 0, st>>>(c->pf_g, c->pf_u, c->ffn_act, c->pf_g, (int)(B * hidden));
      CH_TRY(PT(tl, CRABML_HIP_PFTAP_HID_H, c->pf_g, xb_hid));
      a = quant_rows(c->pf_g, hidden, c->pf_act_hid, c->down[l]);
    }
    CH_TRY(PT(tl && c->qt != CRABML_HIP_F32, CRABML_HIP_PFTAP_HID_ACT, c->pf_act_hid, B * alh.total));
    CH_TRY(gemm(c->down[l], dim, hidden, a, c->pf_tmp, down_deferred ? &down_parts : nullptr, tl ? &fc_down : nullptr,
                tl ? CRABML_HIP_PFTAP_HID_XH : -1, tl ? CRABML_HIP_PFPLAN_KERNEL_DOWN : -1));  // llama2.rs:633-636
    tap.note(l, CRABML_HIP_PFPLAN_DOWN_PARTS, down_deferred ? down_parts : 0);
    note_form(l, CRABML_HIP_PFPLAN_DOWN_F, fc_down);
    CH_TRY(PT(tl, CRABML_HIP_PFTAP_DOWN_TMP, c->pf_tmp, xb_dim));
    CH_TRY(PT(tl && down_deferred && down_parts > 0, CRABML_HIP_PFTAP_DOWN_PARTS, c->pf_split, (size_t)down_parts * xb_dim));
    if (down_deferred) {
      pending_down = true;  // added by the next layer's norm launch
    } else {
      k_res_epi<<<(unsigned)(((size_t)B * dim + 255) / 256), 256, 0, st>>>(c->pf_tmp, c->pf_x, (int)(B * dim), 1);
      CH_TRY(PT(tl, CRABML_HIP_PFTAP_DOWN_X, c->pf_x, xb_dim));
    }
  }
  if (want_logits) {  // final rmsnorm + classifier of the last row only (llama2.rs:274-278, 199-208)
    CH_HIP(dev, hipMemcpyAsync(c->x, c->pf_x + (B - 1) * (size_t)dim, (size_t)dim * 4, hipMemcpyDeviceToDevice, st));
    CH_TRY(PT(true, CRABML_HIP_PFTAP_LAST_X, c->x, (size_t)dim * 4));
    launch_norm_f32(st, c->x, nullptr, (const float*)c->rms_final->ptr, dim, g.rms_norm_eps, c->xn, half);
    CH_TRY(PT(true, CRABML_HIP_PFTAP_CLS_XN, c->xn, (size_t)dim * 4));
    const void* act = c->xn;
    if (c->out_qt != CRABML_HIP_F32) {
      launch_quantize_act(st, c->out_qt, c->xn, (size_t)dim, c->act_dim);
      act = c->act_dim;
    }
    CH_TRY(PT(true, CRABML_HIP_PFTAP_CLS_ACT, act, c->out_qt != CRABML_HIP_F32 ? act_layout(c->out_qt, (size_t)dim).total : (size_t)dim * 4));
    CH_TRY(strict ? launch_gemv_strict(dev, c->output, g.vocab_size, dim, act, 1, c->logits)
                  : launch_gemv(dev, c->output, g.vocab_size, dim, act, 1, c->logits, nullptr));
  }
  CH_HIP(dev, hipGetLastError());
  return 0;
}

// One chunk of the prompt pass.  The f16 GEMM's B' = q * d overflows f16 where the int8 GEMM does not (activations past 65504 -- a
// few massive channels of a real checkpoint; the rows' f16 scales reach about 8.3e6): the writers of B' raise pf_ovf, read here once
// per chunk, and a chunk that raised it is computed again from its token embeddings with the int8 GEMMs -- it overwrites its own KV
// rows and logits; the caller advances kv_len once.  Chunks that do not overflow keep their bits.
// tap_layer >= 0 (crabml_hip_llama_debug_prefill_tap): each pass is enqueued with the copies of that layer switched on, the plan and the
// scratch area started afresh -- after a recomputation they hold the recomputation's
int prefill_chunk(crabml_hip_llama* c, const uint32_t* tokens, size_t B, size_t pos0, bool want_logits, int tap_layer = -1) {
  bool f16w = false;
  auto pass = [&](bool allow_f16w, int recomputed) -> int {
    TapRec& tap = c->pftap;
    if (tap_layer >= 0) tap.arm(tap_layer);
    tap.note(CRABML_HIP_PFPLAN_N_CU, c->dev->n_cu);
    tap.note(CRABML_HIP_PFPLAN_ROWS, (int32_t)B);
    tap.note(CRABML_HIP_PFPLAN_POS0, (int32_t)pos0);
    tap.note(CRABML_HIP_PFPLAN_RECOMPUTED, recomputed);
    const int rc = prefill_chunk_pass(c, tokens, B, pos0, want_logits, allow_f16w, &f16w);
    tap.disarm();
    return rc;
  };
  CH_TRY(pass(true, 0));
  if (!f16w) return 0;
  int h = 0;
  CH_HIP(c->dev, hipMemcpyAsync(&h, c->pf_ovf, sizeof h, hipMemcpyDeviceToHost, c->dev->stream));
  CH_HIP(c->dev, hipStreamSynchronize(c->dev->stream));
  if (h == 0) return 0;
  CH_HIP(c->dev, hipMemsetAsync(c->pf_ovf, 0, sizeof h, c->dev->stream));
  return pass(false, 1);
}

// what crabml_hip_llama_prefill (and the tap of one of its passes) checks before anything is enqueued (llama2.rs:117-122)
int prefill_check(crabml_hip_llama* c, const uint32_t* tokens, size_t n) {
  crabml_hip_device* dev = c->dev;
  if (n == 0) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama prefill: expected at least 1 prompt token");
  for (size_t i = 0; i < n; i++)
    if (tokens[i] >= c->cfg.vocab_size) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: token %u out of range", tokens[i]);
  if (c->kv_len + n > c->cfg.seq_len)
    CH_BAIL(dev, CRABML_HIP_TENSOR_ERROR, "llama: %zu prompt tokens do not fit the kv cache (%zu of %zu used)", n, c->kv_len, c->cfg.seq_len);
  return 0;
}
// rows per pass: 1024 on the fast device (8B shape Q4_0: 31.5k / 38k / 45k / 46k prompt tok/s at 256 / 512 / 1024 / 2048 rows -- the
// narrow GEMMs get their column tiles; the row buffers are ~0.5 GB), 512 on the strict one (its exact attention tiles hold 1024
// positions in LDS), never more than the cache holds
size_t prefill_chunk_rows(const crabml_hip_llama* c) {
  const size_t chunk0 = c->cfg.prefill_chunk ? c->cfg.prefill_chunk : c->dev->strict_order ? 512 : 1024;
  return chunk0 < c->cfg.seq_len ? chunk0 : c->cfg.seq_len;
}

// token, pos, step[, (prefetch sink), serial: the serial set from the host (lazy_ctx_begin) -- five ints, two slots of the ring]
int set_state(crabml_hip_llama* c, size_t token, size_t pos, int step, const unsigned* serial = nullptr) {
  const int st5[5] = {(int)token, (int)pos, step, 0, serial ? (int)*serial : 0};
  const size_t n = serial ? 5 : 3;
  int* st = nullptr;
  CH_TRY(next_state_slot(c, serial ? 2 : 1, &st));
  memcpy(st, st5, n * sizeof(int));
  CH_HIP(c->dev, hipMemcpyAsync(c->state, st, n * sizeof(int), hipMemcpyHostToDevice, c->dev->stream));
  return 0;
}

}  // namespace

extern "C" {

// ---- tensor-parallel communicator (RCCL) ------------------------------------------------------------------
int crabml_hip_tp_get_unique_id(void* id128) {
  Rccl* r = rccl();
  if (!r || !id128) return CRABML_HIP_UNEXPECTED;
  return r->GetUniqueId(id128) == 0 ? 0 : CRABML_HIP_UNEXPECTED;
}

int crabml_hip_tp_comm_create(crabml_hip_device_t* dev, const void* id128, int nranks, int rank, crabml_hip_tp_comm_t** out) {
  if (!dev || !id128 || !out || nranks < 1 || rank < 0 || rank >= nranks) return CRABML_HIP_BAD_INPUT;
  *out = nullptr;
  Rccl* r = rccl();
  if (!r) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "librccl.so could not be loaded");
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  Rccl::IdT id;
  memcpy(&id, id128, sizeof id);
  void* comm = nullptr;
  int rc = r->CommInitRank(&comm, nranks, id, rank);
  if (rc != 0) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "ncclCommInitRank failed: %s", r->GetErrorString ? r->GetErrorString(rc) : "?");
  crabml_hip_tp_comm* c = new crabml_hip_tp_comm();
  c->dev = dev;
  c->nccl = comm;
  c->nranks = nranks;
  c->rank = rank;
  *out = c;
  return 0;
}

int crabml_hip_tp_comm_destroy(crabml_hip_tp_comm_t* comm) {
  if (!comm) return 0;
  if (comm->p2p) {
    (void)hipSetDevice(comm->dev->ordinal);
    (void)hipStreamSynchronize(comm->dev->stream);
    for (int r = 0; r < comm->nranks; r++) {
      if (r == comm->rank || !comm->peer[r]) continue;
      // mapped through IPC (another process): close the mapping; same-process peers (connect_local) are plain pointers owned
      // by their rank and are left alone.  Destroy order: contexts before their group, every rank quiesced.
      if (comm->via_ipc[r]) (void)hipIpcCloseMemHandle(comm->peer[r]);
      (void)hipGetLastError();
    }
    if (comm->inbox) (void)hipFree(comm->inbox);
    delete comm;
    return 0;
  }
  Rccl* r = rccl();
  if (r && comm->nccl) r->CommDestroy(comm->nccl);
  delete comm;
  return 0;
}

// in-place sum over ranks of an F32 buffer's first n elements, on the device stream (the collective the decode
// step issues twice per layer); exposed so the RCCL path can be exercised on its own
int crabml_hip_tp_all_reduce(crabml_hip_tp_comm_t* comm, crabml_hip_buf_t* buf, size_t n) {
  if (!comm || !buf) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = comm->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  if (buf->dtype != CRABML_HIP_F32 || n > buf->n_elems) CH_BAIL(dev, CRABML_HIP_TENSOR_ERROR, "tp_all_reduce: needs an f32 buffer of >= n elements");
  lazy_use(dev, buf);
  CH_TRY(ensure_mem(dev, buf));
  if (comm->p2p) {
    if (!comm->connected) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "tp_all_reduce: the p2p group is not connected");
    if (n > comm->cap) CH_BAIL(dev, CRABML_HIP_TENSOR_ERROR, "tp_all_reduce: %zu elements exceed the inbox rows (%u)", n, comm->cap);
    const unsigned k = comm->host_epoch++;  // every rank issues the same sequence of calls
    k_tp_allreduce<<<(unsigned)((n + 255) / 256), 256, 0, dev->stream>>>((float*)buf->ptr, (int)n, p2p_view(comm), nullptr, 1, (int)(k & 1u),
                                                                       0x40000000u + k, 2);
    CH_HIP(dev, hipGetLastError());
    int fault = 0;
    CH_HIP(dev, hipMemcpyAsync(&fault, comm->fault, sizeof(int), hipMemcpyDeviceToHost, dev->stream));
    CH_HIP(dev, hipStreamSynchronize(dev->stream));
    if (fault) {
      (void)hipMemsetAsync(comm->fault, 0, sizeof(int), dev->stream);  // the group stays usable once the peer shows up
      CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "tp_all_reduce: a peer's partial never arrived (poll timed out)");
    }
    touch(buf);
    return 0;
  }
  Rccl* r = rccl();
  if (!r) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "librccl.so could not be loaded");
  int rc = r->AllReduce(buf->ptr, buf->ptr, n, 7, 0, comm->nccl, dev->stream);
  if (rc != 0) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "ncclAllReduce failed: %s", r->GetErrorString ? r->GetErrorString(rc) : "?");
  touch(buf);
  return 0;
}

// ---- one-shot P2P all-reduce group (the production collective of SURVEY.md 8e; device side: fused_ffn.hpp, TpP2P) --------
int crabml_hip_tp_p2p_create(crabml_hip_device_t* dev, int nranks, int rank, size_t max_elems, crabml_hip_tp_comm_t** out) {
  if (!dev || !out || nranks < 1 || nranks > 8 || rank < 0 || rank >= nranks || max_elems == 0 || max_elems > (1u << 24))
    return CRABML_HIP_BAD_INPUT;
  *out = nullptr;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  crabml_hip_tp_comm* c = new crabml_hip_tp_comm();
  c->dev = dev;
  c->nranks = nranks;
  c->rank = rank;
  c->p2p = true;
  c->cap = (unsigned)((max_elems + 2 + 31) / 32 * 32);  // + the two granules of the vocabulary-split sampler (k_argmax_step_tp)
  c->inbox_bytes = (size_t)TP_SLOTS * nranks * c->cap * 8 + 256;  // + the fault word
  // fine-grained device memory: stores from a peer GPU become visible to a kernel that is already running (the coarse-
  // grained default only promises that at kernel boundaries); plain hipMalloc is the fallback where the flag is refused
  void* p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, c->inbox_bytes, hipDeviceMallocFinegrained);
  c->finegrained = e == hipSuccess;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    e = hipMalloc(&p, c->inbox_bytes);
  }
  if (e == hipSuccess) e = hipMemsetAsync(p, 0, c->inbox_bytes, dev->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
  if (e != hipSuccess) {
    if (p) (void)hipFree(p);
    delete c;
    return hip_fail(dev, e, "tp_p2p_create", __FILE__, __LINE__);
  }
  c->inbox = (unsigned long long*)p;
  c->fault = (int*)((char*)p + (size_t)TP_SLOTS * nranks * c->cap * 8);
  c->peer[rank] = p;
  c->connected = nranks == 1;
  *out = c;
  return 0;
}

// 64 bytes = hipIpcMemHandle_t of this rank's inbox; ship it to every peer (any side channel), then connect
int crabml_hip_tp_p2p_export(crabml_hip_tp_comm_t* comm, void* handle64) {
  if (!comm || !comm->p2p || !handle64) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = comm->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  hipIpcMemHandle_t h;
  CH_HIP(dev, hipIpcGetMemHandle(&h, comm->inbox));
  memcpy(handle64, &h, 64);
  return 0;
}

// handles: nranks x 64 bytes in rank order (this rank's own entry is ignored)
int crabml_hip_tp_p2p_connect(crabml_hip_tp_comm_t* comm, const void* handles) {
  if (!comm || !comm->p2p || !handles) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = comm->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  if (comm->connected && comm->nranks > 1) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "tp_p2p_connect: already connected");
  for (int r = 0; r < comm->nranks; r++) {
    if (r == comm->rank) continue;
    hipIpcMemHandle_t h;
    memcpy(&h, (const char*)handles + (size_t)r * 64, 64);
    void* p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return hip_fail(dev, e, "hipIpcOpenMemHandle (peer inbox)", __FILE__, __LINE__);
    comm->peer[r] = p;
    comm->via_ipc[r] = true;
  }
  comm->connected = true;
  return 0;
}

// the same wiring for ranks that live in ONE process (one HipTensorDevice / stream per rank, possibly on the same GPU):
// the inboxes are plain device pointers, no IPC handle is involved
int crabml_hip_tp_p2p_connect_local(crabml_hip_tp_comm_t* const* comms, int n) {
  if (!comms || n < 1 || n > 8) return CRABML_HIP_BAD_INPUT;
  for (int r = 0; r < n; r++)
    if (!comms[r] || !comms[r]->p2p || comms[r]->nranks != n || comms[r]->rank != r || comms[r]->cap != comms[0]->cap)
      return CRABML_HIP_BAD_INPUT;
  for (int r = 0; r < n; r++) {
    for (int p = 0; p < n; p++) {
      if (p == r) continue;
      if (comms[p]->dev->ordinal != comms[r]->dev->ordinal) {  // another GPU of this process: map it
        (void)hipSetDevice(comms[r]->dev->ordinal);
        hipError_t e = hipDeviceEnablePeerAccess(comms[p]->dev->ordinal, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return hip_fail(comms[r]->dev, e, "hipDeviceEnablePeerAccess", __FILE__, __LINE__);
        (void)hipGetLastError();
      }
      comms[r]->peer[p] = comms[p]->inbox;
    }
    comms[r]->connected = true;
  }
  return 0;
}

}  // extern "C"

// ---- creating a context: validate, decide, retain, allocate, initialise, capture (llama_create_impl calls them in this order) ----

// what validation learns of a model: the facts decide_step and the later stages work from
struct ModelFacts {
  int tp = 1;
  bool p2p_comm = false;  // the group is the P2P kind: the wo / ffn_down epilogue can host the collective
  bool tp_dry = false;    // CRABML_HIP_LLAMA_TP_DRY_RUN: a lone rank that skips the all-reduces
  bool qwen2 = false, gemma = false;
  size_t hd = 0, n_heads_l = 0, n_kv_l = 0, dim_l = 0, kv_dim_l = 0, hidden_l = 0;  // local (per-rank) geometry
  const crabml_hip_buf* outw = nullptr;                                             // the classifier: output.weight, else the embedding
  uint32_t wt = 0, out_wt = 0, qt = 0, out_qt = 0;  // weight type of the layers / the classifier, and their vec_dot_rhs_dtype
  bool mixed = false;                               // some layer matrix has another type than wq[0] (with the same rhs type)
  // every deviating tensor is one the layers' K-quant body takes beside its own format (its row of the table: k_body_of / KBody::VAlt)
  // -- attn_v or ffn_down, and attn_output too where the alternates do not come whole -- in one of the row's formats
  bool family_ok = true;
  bool mix_v_down_q6k = true;  // ... and they come whole: an attn_v / ffn_down in Q6_K inside a Q4_K / Q5_K layer (the *_K_M recipe)
  bool split_vocab = false;
  size_t vocab_l = 0;
};

// the configuration, the architecture and its biases, and that every weight is there
static int validate_config(crabml_hip_device_t* dev, const crabml_hip_llama_config_t& g, const crabml_hip_llama_weights_t* w,
                           const crabml_hip_llama_arch_t* arch, ModelFacts* f) {
  const int tp = f->tp = g.tp_size > 1 ? g.tp_size : 1;
  if (!g.n_heads || !g.n_kv_heads || !g.n_layers || g.embedding_dim % g.n_heads || g.n_heads % g.n_kv_heads)
    CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: inconsistent head configuration");
  // (asked before the divisibility checks: Gemma-2B has ONE kv head, which no tp_size > 1 divides -- the answer is "not implemented")
  if (arch && arch->architecture == CRABML_HIP_ARCH_GEMMA && tp > 1)
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "gemma: tensor parallelism is not implemented");
  if (tp > 8 || g.tp_rank < 0 || g.tp_rank >= tp || g.n_kv_heads % tp || g.hidden_dim % tp)
    CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: tp_size %d must divide n_kv_heads and hidden_dim (and be <= 8)", tp);
  if (g.tp_comm) {
    const crabml_hip_tp_comm* m = (const crabml_hip_tp_comm*)g.tp_comm;
    if (m->p2p && (!m->connected || m->nranks != tp || m->rank != g.tp_rank || m->cap < g.embedding_dim || m->dev != dev))
      CH_BAIL(dev, CRABML_HIP_BAD_INPUT,
              "llama: the p2p group must be connected, match tp_size / tp_rank, live on this device and hold rows of >= embedding_dim");
    f->p2p_comm = m->p2p;
  }
  f->tp_dry = tp > 1 && !g.tp_comm && (g.flags & CRABML_HIP_LLAMA_TP_DRY_RUN);
  // the F32 KV cache pairs head h with kv head h % n_kv (the batch_matmul broadcast quirk): those sets are not
  // contiguous head slices, so a GQA model shards by heads only with the F16 cache (h / (n_heads / n_kv))
  if (tp > 1 && !g.use_f16_kv_cache && g.n_heads != g.n_kv_heads)
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama: tensor-parallel GQA needs the f16 kv cache");
  const size_t hd = f->hd = g.embedding_dim / g.n_heads;
  f->n_heads_l = g.n_heads / tp;
  f->n_kv_l = g.n_kv_heads / tp;
  f->dim_l = f->n_heads_l * hd;
  f->kv_dim_l = f->n_kv_l * hd;
  f->hidden_l = g.hidden_dim / tp;
  if (g.embedding_dim % 32 || f->hidden_l % 32 || f->dim_l % 32 || (hd & 1) || hd > 256 || (g.rope_dim & 1) || g.rope_dim > hd || !g.seq_len)
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama fused path: needs dim, local dims % 32 == 0, even head_dim <= 256, even rope_dim");
  if (g.embedding_dim > 12288)  // k_norm_quant keeps the row in 64 KiB of LDS
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama fused path: embedding_dim %zu > 12288", g.embedding_dim);
  if (!w->token_embed || !w->rms_final_weight || !w->wq || !w->wk || !w->wv || !w->wo || !w->ffn_gate_weight ||
      !w->ffn_down_weight || !w->ffn_up_weight || !w->rms_att_weight || !w->rms_ffn_weight)
    CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: missing weights");
  // the architecture (model.rs:22-27): Llama; Qwen2 = Llama + q / k / v biases + NEOX rope (llama2.rs:283-351); Gemma = Llama with the
  // embedding scaled by sqrt(dim), NEOX rope and GELU (llama2.rs:455-524; its classifier is whatever the weights say, as everywhere)
  const uint32_t archv = arch ? arch->architecture : (uint32_t)CRABML_HIP_ARCH_LLAMA;
  const bool qwen2 = f->qwen2 = archv == CRABML_HIP_ARCH_QWEN2, gemma = f->gemma = archv == CRABML_HIP_ARCH_GEMMA;
  if (archv == CRABML_HIP_ARCH_PHI2) CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama: architecture %u (Phi2) has no decode step here", archv);
  if (archv != CRABML_HIP_ARCH_LLAMA && !qwen2 && !gemma) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: unknown architecture %u", archv);
  if (gemma && (arch->bq || arch->bk || arch->bv)) CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "gemma: there is no decode step with q / k / v biases");
  if (!qwen2 && arch && (arch->bq || arch->bk || arch->bv)) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: a Llama model has no q / k / v biases");
  if (qwen2) {
    if (tp > 1) CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "qwen2: tensor parallelism is not implemented");
    if (!arch->bq || !arch->bk || !arch->bv) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "qwen2: missing q / k / v biases");
    for (size_t l = 0; l < g.n_layers; l++) {
      const crabml_hip_buf* b[3] = {arch->bq[l], arch->bk[l], arch->bv[l]};
      const size_t n[3] = {f->dim_l, f->kv_dim_l, f->kv_dim_l};
      for (int j = 0; j < 3; j++)
        if (!b[j] || b[j]->dtype != CRABML_HIP_F32 || b[j]->n_elems != n[j])
          CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "qwen2: layer %zu: the %c bias must be an f32 vector of %zu elements", l, "qkv"[j], n[j]);
    }
  }
  return 0;
}

// type and shape of every weight.  Fused kernels exist for Q4_0 / Q8_0 / Q4_1 and the K-quant bodies (KBodies); a classifier of another format --
// llama.cpp's "Q4_0" files keep output.weight in Q6_K -- does not take the layers off them: the final segment quantizes the
// normalized row for the classifier's own rhs type.
static int validate_weights(crabml_hip_device_t* dev, const crabml_hip_llama_config_t& g, const crabml_hip_llama_weights_t* w, ModelFacts* f) {
  const int tp = f->tp;
  const size_t dim = g.embedding_dim, dim_l = f->dim_l, kv_dim_l = f->kv_dim_l, hidden_l = f->hidden_l;
  const crabml_hip_buf* outw = f->outw = w->output_weight ? w->output_weight : w->token_embed;
  const uint32_t wt = f->wt = w->wq[0]->dtype, out_wt = f->out_wt = outw->dtype;
  const uint32_t qt = f->qt = vec_dot_rhs_dtype(wt), out_qt = f->out_qt = vec_dot_rhs_dtype(out_wt);
  if (qt == 0xffffffffu || out_qt == 0xffffffffu)
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama: weight dtype %u / classifier dtype %u has no matmul_vec", wt, out_wt);
  {
    const size_t be = block_elems(wt) > block_elems(qt) ? block_elems(wt) : block_elems(qt);
    const size_t obe = block_elems(out_wt) > block_elems(out_qt) ? block_elems(out_wt) : block_elems(out_qt);
    if (dim % be || dim_l % be || hidden_l % be || dim % obe)
      CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama: dim / local dims are not multiples of the %zu-element blocks of dtype %u", be, wt);
  }
  // (a Q5_0 tensor: BlockFmt<Q5_0>::load finds the d plane (qh plane - qs plane) / 4 bytes behind the qh plane, which holds only while
  // the qs plane is n * 16 bytes exactly -- a layout with padding there is refused here, not read out of bounds)
  auto check = [&](const crabml_hip_buf* b, size_t m, size_t k, uint32_t t) {
    return b && b->dtype == t && b->n_elems == m * k && (block_elems(t) == 1 || b->k == k) &&
           (t != CRABML_HIP_Q5_0 || b->wl.off_scale == b->wl.n_blocks * 16);
  };
  // a layer's matrices may differ in GGML type (llama.cpp's *_K_M files: attn_v / ffn_down in Q6_K on some layers) as
  // long as they share the rhs type (buf/api.rs:142-159: every K-quant takes Q8_K): such a model runs the per-op
  // segments, each GEMV picking its kernel by the tensor's own dtype -- unless every deviating tensor is one the body takes (its
  // row: the *_K_M recipes of a Q4_K / Q5_K body, the Q3_K and the Q2_K recipe families; wo: attn_output, which may deviate beside
  // attn_v and ffn_down where the alternates do not come whole)
  const KBodyRow* const body = k_body_of(wt);
  auto check_w = [&](const crabml_hip_buf* b, size_t m, size_t k, bool v_or_down, bool wo = false) {
    if (!b) return false;
    if (b->dtype != wt) {
      if (vec_dot_rhs_dtype(b->dtype) != qt || k % block_elems(b->dtype)) return false;
      f->mixed = true;
      const bool taken = body && (v_or_down || (wo && !body->v_whole)) && body->takes(b->dtype);
      if (!taken) f->family_ok = false;
      if (!(taken && body->v_whole)) f->mix_v_down_q6k = false;
    }
    return check(b, m, k, b->dtype);
  };
  for (size_t l = 0; l < g.n_layers; l++) {
    if (!check_w(w->wq[l], dim_l, dim, false) || !check_w(w->wk[l], kv_dim_l, dim, false) || !check_w(w->wv[l], kv_dim_l, dim, true) ||
        !check_w(w->wo[l], dim, dim_l, false, true) || !check_w(w->ffn_gate_weight[l], hidden_l, dim, false) ||
        !check_w(w->ffn_up_weight[l], hidden_l, dim, false) || !check_w(w->ffn_down_weight[l], dim, hidden_l, true) ||
        !check(w->rms_att_weight[l], 1, dim, CRABML_HIP_F32) || !check(w->rms_ffn_weight[l], 1, dim, CRABML_HIP_F32))
      CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED,
              "llama fused path: layer %zu weights have an unexpected shape, or dtypes that do not share one rhs dtype (tp=%d)", l, tp);
  }
  // the classifier split by vocabulary: this rank holds rows [tp_rank V / tp, (tp_rank + 1) V / tp)
  f->split_vocab = tp > 1 && (g.flags & CRABML_HIP_LLAMA_TP_SPLIT_VOCAB) != 0;
  if (f->split_vocab) {
    if (!w->output_weight || g.vocab_size % tp)
      CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: the vocabulary split needs an untied output.weight and vocab_size %% tp_size == 0");
    if (g.tp_comm && !f->p2p_comm)
      CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama: the vocabulary split exchanges its arg-max pairs through a P2P group (crabml_hip_tp_p2p_*)");
  }
  f->vocab_l = f->split_vocab ? g.vocab_size / tp : g.vocab_size;
  if (!check(outw, f->vocab_l, dim, out_wt) || !check(w->rms_final_weight, 1, dim, CRABML_HIP_F32) || w->token_embed->n_elems != g.vocab_size * dim)
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama fused path: classifier / final norm / embedding dtype or shape");
  return 0;
}

// the three tuning hooks of the split-KV attention (tools/flash_sweep.py; armed like ASSUME_CUS), as values
struct FlashHooks {
  int slices = 0;             // CRABML_HIP_FLASH_SLICES: slices per kv head in the grid (0 = not set)
  int min_rows = 0;           // CRABML_HIP_FLASH_MIN_ROWS (0 = not set)
  size_t ticket_until = 768;  // CRABML_HIP_FLASH_TICKET_UNTIL: 0 = never
};
static FlashHooks read_flash_hooks() {
  FlashHooks h;
  h.slices = test_hook_int("CRABML_HIP_FLASH_SLICES", 0);
  h.min_rows = test_hook_int("CRABML_HIP_FLASH_MIN_ROWS", 0);
  if (const char* e = test_hook("CRABML_HIP_FLASH_TICKET_UNTIL")) h.ticket_until = (size_t)atol(e);
  return h;
}

// The one question decide_step asks of the device: does kernel `fn` get `bytes` of dynamic LDS?  Yes when that is under `cap` and, if
// it is above `granted` (what a launch gets without asking), the kernel's limit could be raised -- which the record-only device refuses.
constexpr size_t LDS_CAP = 150 * 1024, LDS_NO_CAP = ~(size_t)0;
static bool lds_fits(const crabml_hip_device* dev, const void* fn, size_t bytes, size_t cap, size_t granted) {
  if (bytes > cap) return false;
  if (bytes <= granted) return true;
  const bool ok = raise_dyn_lds(dev, fn, (int)bytes) == hipSuccess;
  (void)hipGetLastError();
  return ok;
}

// a cache whose positions k_attn's score row (one workgroup per head, the whole row and q in LDS) cannot span
static bool past_k_attn_row(size_t seq, size_t hd) { return k_attn_lds_bytes(seq, hd) > K_ATTN_LDS; }

// The attention forms of a plan.  Each kernel's limit is asked for where the plan first needs that kernel, in this order: the exact
// softmax, k_attn_pv_split, k_attn_flash, its ticket form, k_attn_flash_rows, k_attn_s -- a refusal turns that form off, nothing else.
static void decide_attention(const crabml_hip_device* dev, const crabml_hip_llama_config_t& g, const ModelFacts& f, const FlashHooks& hooks,
                             StepPlan* p) {
  const auto has = [&](int bits) { return (g.flags & bits) != 0; };
  const int grp = (int)(f.n_heads_l / f.n_kv_l), hd = (int)f.hd, n_kv_l = (int)f.n_kv_l;
  const size_t seq = g.seq_len;
  const bool kv16 = g.use_f16_kv_cache != 0, q81 = f.qt == CRABML_HIP_Q8_1;
  // One predicate per use.  The decode step's kernels (k_attn_flash; k_attn_scores / k_attn_softmax / k_attn_pv) serve every group up to 8;
  // the prompt pass's (k_attn_flash_rows here, the tile and long-rows kernels through their own lists) serve 1, 2, 4 and 8 only -- any
  // other group keeps its prompt on the per-(head, row) kernel.  That kernel's score row ends at 64 KiB, so in a cache past
  // past_k_attn_row() k_attn_flash_rows (group-agnostic: kv head = head / (n_heads / n_kv)) takes groups 3, 5, 6 and 7 as well; under
  // that bound they stay where the launch pins hold them.
  const bool long_cache = kv16 && hd % 32 == 0 && !has(CRABML_HIP_LLAMA_NO_LONG_ATTENTION);
  const bool long_geom = long_cache && grp >= 1 && grp <= 8;
  const bool rows_geom = past_k_attn_row(seq, f.hd) ? long_geom : long_cache && exact_rows_group(grp);
  // the exact kernels: the softmax kernels keep a head's score row in LDS -- rows past 16384 positions need the raised limit, rows
  // past ~38000 do not fit at all (the step then stays on the one-workgroup-per-head kernel)
  p->exact_long_ok = long_geom && seq % 8 == 0 && lds_fits(dev, (const void*)k_attn_softmax<16>, seq * 4, LDS_CAP, 64 * 1024) &&
                     lds_fits(dev, (const void*)k_attn_softmax<4>, seq * 4, LDS_CAP, 64 * 1024);
  p->pv_split = p->exact_long_ok && !has(CRABML_HIP_LLAMA_NO_PV_PRODUCER_WAVES) && [&] {
    const PvSplitKernel pv = pv_split_kernel(grp);
    return pv.fn != nullptr && lds_fits(dev, (const void*)pv.fn, pv.lds, LDS_NO_CAP, 0);
  }();
  // the fast step's long-context attention: split-KV with f32 accumulation (k_attn_flash) unless the exact chain is asked for
  // (k_attn_flash reads the cache rows only -- head_dim halves each --, so any seq_len will do: a cache of 1001 positions must not
  // fall back to one workgroup per head, 45 us per layer at 900 positions)
  const bool want_flash = long_geom && !dev->strict_order && !has(CRABML_HIP_LLAMA_EXACT_ATTENTION);
  p->flash_ticket = want_flash && has(CRABML_HIP_LLAMA_FLASH_TICKET);
  const FlashFn fn = want_flash ? flash_kernel(grp, hd, q81, p->flash_ticket) : nullptr;
  p->attn_flash = fn != nullptr && lds_fits(dev, (const void*)fn, flash_lds_bytes(grp, hd), LDS_NO_CAP, 0);
  if (p->attn_flash) {
    const int S = dev->n_cu / n_kv_l;
    p->flash_S = hooks.slices >= 1 && hooks.slices <= FLASH_MAX_SLICES ? hooks.slices : S < 1 ? 1 : S > FLASH_MAX_SLICES ? FLASH_MAX_SLICES : S;
    if (hooks.min_rows >= 8 && hooks.min_rows <= 65536) p->flash_min_rows = hooks.min_rows;
    // Below ~768 cached positions the merge inside the launch (last-arriving workgroup of a kv head, ticket word) beats the
    // second launch -- 7.4 vs 5.1 + 4.1 us per layer at 128 positions, 8.7 vs 10.0 at 512, 10.8 vs 9.95 at 1024
    // (profiles/r05_flash_ticket_sweep.md; same partials, same merge order: bit-identical): a third graph variant serves that range.
    const FlashFn tfn = flash_kernel(grp, hd, q81, true);
    if (!p->flash_ticket && hooks.ticket_until > 0 && tfn != nullptr && lds_fits(dev, (const void*)tfn, flash_lds_bytes(grp, hd), LDS_NO_CAP, 0))
      p->flash_ticket_until = hooks.ticket_until;
    // the prompt pass's causal attention of the fast step (k_attn_flash_rows): 70 KB of LDS at head_dim 128
    p->attn_flash_rows =
        rows_geom && flash_rows_kernel(hd) != nullptr && lds_fits(dev, (const void*)flash_rows_kernel(hd), flash_rows_lds_bytes(hd), LDS_NO_CAP, 0);
  }
  p->attn_long_ok = p->exact_long_ok || p->attn_flash;
  // the exact kernels: measured crossover on MI355X (Llama-3-8B shape) ~200-220.  k_attn_flash + merge overtake the staged one-workgroup
  // kernel between 64 and 96 cached positions (8B shape, per layer: 51.0 vs 51.6 us at 64, 52.2 vs 51.4 at 96, 59.0 vs 51.8 at 224;
  // profiles/r04_flash_sweep.log)
  p->attn_long_from = g.attn_long_from ? g.attn_long_from : p->attn_flash ? 96 : 224;
  // short-context attention with K / V staged through LDS (f16 cache): variant 0 serves positions < S
  if (kv16 && hd % 8 == 0 && !has(CRABML_HIP_LLAMA_NO_STAGED_ATTENTION)) {
    const size_t S = p->attn_long_ok && p->attn_long_from < seq ? p->attn_long_from : seq;
    const size_t lds = attn_s_lds_bytes((int)S, hd);
    if (lds_fits(dev, (const void*)attn_s_kernel(hd), lds, LDS_CAP, 0)) {
      p->attn_s_rows = (int)S;
      p->attn_s_lds = lds;
    }
  }
}

// The longest cache a context is created with: the context length of the Qwen2.5 / Mistral / Llama-3.1 files this is for, inside the
// 38400 positions (LDS_CAP) of the exact softmax kernels.  tests/test_hip_fused.py::test_fused_errors holds a fast f16 context of
// 65536 positions to a refusal: going further has to touch that test.
constexpr size_t MAX_SEQ_LEN = 32768;

// Why a plan cannot serve its cache (nullptr: it can).  Up to the 64 KiB score row of k_attn every plan can: that kernel is what
// every other form falls back to.  Past it a context exists only if no launch its plan can choose is k_attn with a cache-sized row:
// the decode step goes k_attn_s -> the long-context kernels, the prompt pass goes k_attn_flash_rows (short passes: the tile kernel, or
// k_attn with a pass-sized row) or the exact tile / long-rows kernels.  The kernels' own limits are decide_attention's; this reads its words.
// plan == nullptr: the clauses the configuration alone settles, asked before decide_step -- which raises kernels' LDS limits -- runs
// for a context that cannot exist.
static const char* long_cache_refusal(const crabml_hip_llama_config_t& g, const ModelFacts& f, const StepPlan* plan) {
  if (!past_k_attn_row(g.seq_len, f.hd)) return nullptr;
  if (g.seq_len > MAX_SEQ_LEN) return "more positions than the limit";
  if (f.tp > 1) return "tensor-parallel ranks keep the one-workgroup-per-head attention within reach";
  if (!g.use_f16_kv_cache) return "an f32 kv cache has no long-context attention kernels";
  if (!plan) return nullptr;
  const StepPlan& p = *plan;
  if (!p.attn_long_ok) return "the decode step has no long-context attention (flags, head_dim, a group above 8, seq_len % 8 on the exact kernels)";
  if (p.attn_long_from >= g.seq_len) return "attn_long_from leaves the whole cache to the short-context attention";
  if (p.attn_s_rows <= 0) return "the decode step's short-context attention would need the whole score row in LDS (k_attn_s is off or does not fit)";
  const bool exact_rows = p.exact_long_ok && exact_rows_group((int)(f.n_heads_l / f.n_kv_l)) && exact_rows_on(g);
  if (!p.attn_flash_rows && !exact_rows)
    return "the prompt pass has no attention kernel for this cache (exact kernels: groups 1, 2, 4, 8, seq_len % 8 == 0, tile attention on)";
  return nullptr;
}

// What a context runs (StepPlan), from values: the configuration, the device's mode and size, and what validation found.  The one
// place that decides it; crabml_hip_debug_step_plan reads it out, tests/test_step_plan.py holds the table.  Every clause that more
// than one decision needs is named once.  The LDS-dependent choices fall back where they always did: the ordered five launches to the
// per-op segments, the ordered Q4_K launches to what an unordered context of the flags gets (on a strict device: per-op).
static StepPlan decide_step(const crabml_hip_device* dev, const crabml_hip_llama_config_t& g, const ModelFacts& f, const FlashHooks& hooks) {
  const auto has = [&](int bits) { return (g.flags & bits) != 0; };
  const bool strict = dev->strict_order;
  const int n_cu = dev->n_cu, tp = f.tp, dim = (int)g.embedding_dim, dim_l = (int)f.dim_l, hidden_l = (int)f.hidden_l, hd = (int)f.hd;
  const uint32_t wt = f.wt;
  // Q5_0 follows Q4_0 and Q5_1 follows Q4_1 in every clause below, on one device: a tensor-parallel rank of either keeps the per-op
  // segments (none of the tensor-parallel launch forms is built for them)
  const bool q5_fmt = wt == CRABML_HIP_Q5_0 || wt == CRABML_HIP_Q5_1;
  const bool like_q4_0 = wt == CRABML_HIP_Q4_0 || wt == CRABML_HIP_Q5_0, like_q4_1 = wt == CRABML_HIP_Q4_1 || wt == CRABML_HIP_Q5_1;
  const bool fused_fmt = wt == CRABML_HIP_Q4_0 || wt == CRABML_HIP_Q8_0 || wt == CRABML_HIP_Q4_1 || (q5_fmt && tp == 1);  // a dot of one term per block
  const bool chunks_resident = dim / 32 <= n_cu;  // every workgroup of a wo / ffn_down gather must be resident
  // the K-quant norm epilogue (Q8_K planes out of wo / ffn_down): what every Q4_K form below builds on, and the ONLY form an EPI_ONLY
  // body (its row of the table, k_body_of) is built in -- such a context that misses a clause of it (a classifier with another rhs,
  // NO_NORM_EPILOGUE, a dim that is no multiple of 256, chunks that are not resident) runs the per-op segments
  const KBodyRow* const body = k_body_of(wt);
  const bool k_body = body != nullptr, k_body_epi_only = k_body && body->epi_only;
  const bool k_epilogue_eligible = k_body && f.out_qt == CRABML_HIP_Q8_K && tp == 1 && !has(CRABML_HIP_LLAMA_NO_NORM_EPILOGUE) &&
                                   dim % 256 == 0 && chunks_resident;
  const bool k_fusion = !has(CRABML_HIP_LLAMA_NO_KQUANT_FUSION);
  // the K-quant fused kernels take the tensors a body's row admits beside its own format (f.family_ok: the *_K_M recipes, the Q3_K and
  // the Q2_K recipe families), but only in the norm-epilogue form.  A body with any other deviation: per-op segments.
  const bool mix_fused = f.mixed && f.family_ok && !strict && k_epilogue_eligible && k_fusion;

  // Strict order, one device, Q4_0 / Q8_0 / Q4_1: the fused launches in their block-ordered form (7 per layer: norm + quantize stay
  // their own launches).  The term tables must fit LDS: 64 rows of gate | up (k_gateup_q_ord, raised past 60 KiB), a workgroup's 16 / 32
  // rows of ffn_down (k_gemv_res_nq_ord keeps the default limit; wo's rows are at most 12288 long: 32 x 388 floats, inside it).
  const auto ord5_fits = [&] {
    const void* fn = nullptr;  // (enqueue_segment_t launches k_gateup_q_ord<FMT> of the same weight type)
    with_const_else<CRABML_HIP_Q4_0, CRABML_HIP_Q8_0, CRABML_HIP_Q5_0, CRABML_HIP_Q5_1, CRABML_HIP_Q4_1>(
        (int)wt, [&](auto fmt) { fn = (const void*)k_gateup_q_ord<decltype(fmt)::value>; });
    return nq_ord_lds_bytes(hidden_l / 32, chunk_split(g.flags, hidden_l, dim, n_cu)) <= 60 * 1024 &&
           lds_fits(dev, fn, gateup_q_ord_lds_bytes(dim / 32), LDS_CAP, 60 * 1024);
  };
  const bool ord5 = strict && fused_fmt && tp == 1 && ord5_fits() && !f.mixed;  // (a mixed file: per-op segments)
  // Strict order, Q4_K layers on one device (a *_K_M mix too: its Q6_K rows leave the same records, rows_terms_q6k): the five launches
  // of the fast Q4_K step in their ORDERED form -- nine f32 terms per super-block parked in LDS and added in super-block order, the
  // reference's norm order in the wo / ffn_down epilogue; bit-identical to the per-op segments they replace (16 launches per layer).
  // Both QOUT forms of gate | up and every <SPLIT, QIN> of wo / ffn_down are raised: q8k_producers and the splits are the launches' own.
  const auto ordk_fits = [&] {  // (wo never runs x_only here: k_norm_in is off on a strict-order device)
    if (dev->dry) return true;  // (record-only device: nothing to raise, nothing launched)
    const size_t gu = q8k_ord_lds_bytes(dim, 64);
    const size_t dn = q8k_ord_lds_bytes(hidden_l, 32 / chunk_split(g.flags, hidden_l, dim, n_cu));
    const size_t wo = q8k_ord_lds_bytes(dim_l, 32 / chunk_split(g.flags, dim_l, dim, n_cu));
    const size_t nq = dn > wo ? dn : wo;
    bool fits = gu <= LDS_CAP && nq <= LDS_CAP;
    for (int qout = 0; qout < 2; qout++) fits = fits && lds_fits(dev, (const void*)gateup_k_kernel(qout != 0, true, false), gu, LDS_CAP, 48 * 1024);
    for (int split = 1; split <= 2; split++)
      for (int qin = 1; qin <= 2; qin++) fits = fits && lds_fits(dev, (const void*)nq_ord_k_kernel(split, qin), nq, LDS_CAP, 48 * 1024);
    return fits;
  };
  const bool ordk = strict && wt == CRABML_HIP_Q4_K && k_epilogue_eligible && k_fusion && !has(CRABML_HIP_LLAMA_NO_RHS_PROLOGUE) && (!f.mixed || f.mix_v_down_q6k) &&
                    dim_l % 256 == 0 && hidden_l % 256 == 0 && ordk_fits();
  // the fast K-quant segments: Q4_K always; an EPI_ONLY body in the norm-epilogue form (none has an ordered form: a strict-order device
  // keeps them on the per-op segments); Q4_1 when it cannot take the five launches (a classifier of another format) or for the A/B flag
  const bool fast_k = !strict && (!f.mixed || mix_fused) && k_fusion &&
                      ((k_body && (!k_body_epi_only || k_epilogue_eligible)) || (fused_fmt && like_q4_1 && (f.out_wt != wt || (wt == CRABML_HIP_Q4_1 && has(CRABML_HIP_LLAMA_Q4_1_SEGMENTS)))));
  // per-op launches: a strict-order device without an ordered form, a weight format without fused kernels, a mix they do not take
  const bool per_op = (strict && !ord5) || !fused_fmt || (f.mixed && !mix_fused);

  StepPlan p;
  p.path = ordk || fast_k ? SegPath::FusedK : per_op ? SegPath::PerOp : SegPath::Fused5;
  p.ordered = ord5 || ordk;
  // (So Fused5 && !ordered says: Q4_0 / Q8_0 / Q4_1 layers, no mix, not a strict-order device -- Fused5 needs fused_fmt and, on a
  // strict device, ord5.  FusedK && !ordered says: not a strict-order device.  The tap hooks and the forms below rely on both.)
  const bool five = p.path == SegPath::Fused5;
  const bool fast_q40_q80 = !p.ordered && (like_q4_0 || wt == CRABML_HIP_Q8_0);  // beside norm_epi: the hop-free forms' step
  // tp > 1: the epilogue also hosts the collective when the group is the P2P kind (or in the collective-free dry run).  Not for the
  // K-quant segments -- a Q4_1 body with a classifier of another format runs them: their wo / ffn_down launches host neither the norm
  // epilogue nor the collective, so over a P2P group the stand-alone all-reduce launch must run.
  p.norm_epi = five && (tp == 1 || f.p2p_comm || f.tp_dry) && !has(CRABML_HIP_LLAMA_NO_NORM_EPILOGUE) && chunks_resident;
  p.norm_epi_k = p.path == SegPath::FusedK && k_epilogue_eligible;
  p.defer_norm = p.norm_epi && tp == 1 && fast_q40_q80 && !has(CRABML_HIP_LLAMA_EXACT_NORM);
  // A tensor-parallel rank's gate/up: hidden / tp / 32 workgroups of 32 rows would leave most CUs idle.  h stays f32 from workgroups
  // of `gu_rows` rows (the largest even divisor of the rank's rows, at most 32, that gives at least one workgroup per CU) and
  // ffn_down quantizes it in its prologue.  (Never picked on the record-only device.)
  const auto pick_gu_rows = [&] {
    for (int r = 30; r >= 2; r -= 2)
      if (hidden_l % r == 0 && hidden_l / r >= n_cu && hidden_l / r <= 2 * n_cu) return q8_0_lds_bytes(hidden_l / 32) <= 60 * 1024 ? r : 0;
    return 0;
  };
  p.gu_rows = p.norm_epi && tp > 1 && fast_q40_q80 && !has(CRABML_HIP_LLAMA_NO_H_CONSUMER_QUANT) && hidden_l % 32 == 0 &&
                      hidden_l / 32 * 2 <= n_cu && !dev->dry
                  ? pick_gu_rows()
                  : 0;
  p.q8k_producers = p.norm_epi_k && !has(CRABML_HIP_LLAMA_NO_RHS_PROLOGUE | CRABML_HIP_LLAMA_NO_Q8K_PRODUCERS) && dim_l % 256 == 0 &&
                    hidden_l % 256 == 0 && (hd == 64 || hd == 128 || hd == 256) && hidden_l / 32 <= 2 * n_cu;
  // the fast Q4_K step: wo leaves x only, gate | up normalizes and quantizes the row itself (k_gateup_k_lds<.., NORMIN>; the same bits)
  p.k_norm_in = p.q8k_producers && !p.ordered && dim / 256 <= 32 &&
                !has(CRABML_HIP_LLAMA_NO_K_NORM_IN | CRABML_HIP_LLAMA_SPLIT_CHUNKS_ALWAYS | CRABML_HIP_LLAMA_SPLIT_CHUNKS_NEVER);
  decide_attention(dev, g, f, hooks, &p);
  return p;
}

// a fresh context with its identity, geometry and plan; on a live device, the pinned state ring (and lazy.hip's logits copy)
static int new_context(crabml_hip_device_t* dev, const crabml_hip_llama_config_t& g, const ModelFacts& f, const StepPlan& plan, bool ext_kv,
                       crabml_hip_llama** out) {
  crabml_hip_llama* c = new crabml_hip_llama();
  c->dev = dev;
  if (!dev->dry && hipHostMalloc((void**)&c->h_state, (crabml_hip_llama::H_STATE_SLOTS * 4 + 4) * sizeof(int), hipHostMallocDefault) != hipSuccess) {
    delete c;
    CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: hipHostMalloc of the state staging ring failed");
  }
  c->cfg = g;
  c->wtype = f.wt;
  c->plan = plan;
  if (ext_kv && !dev->dry) {
    static const bool on = [] { const char* e = getenv("CRABML_HIP_LAZY_NO_HOST_LOGITS"); return !(e && e[0] == '1'); }();
    if (on && hipHostMalloc((void**)&c->host_logits, g.vocab_size * 4 + 64, hipHostMallocDefault) == hipSuccess)
      memset(c->host_logits + g.vocab_size, 0, 64);
    else
      c->host_logits = nullptr;
    (void)hipGetLastError();
  }
  c->qt = f.qt;
  c->out_qt = f.out_qt;
  c->tp = f.tp;
  c->tp_rank = g.tp_rank;
  c->comm = (crabml_hip_tp_comm*)g.tp_comm;
  c->tp_dry = f.tp_dry;
  if (f.p2p_comm) c->tp_salt = (++c->comm->sessions) * 0x9E3779B1u;
  c->split_vocab = f.split_vocab;
  c->vocab_l = (int)f.vocab_l;
  c->vocab_off = f.split_vocab ? (int)(f.vocab_l * (size_t)g.tp_rank) : 0;
  c->hd = (int)f.hd;
  c->npairs = (int)(g.rope_dim / 2);
  c->n_heads_l = (int)f.n_heads_l;
  c->n_kv_l = (int)f.n_kv_l;
  c->dim_l = (int)f.dim_l;
  c->kv_dim_l = (int)f.kv_dim_l;
  c->hidden_l = (int)f.hidden_l;
  c->qwen2 = f.qwen2;
  c->gemma = f.gemma;
  c->ext_kv = ext_kv;
  *out = c;
  return 0;
}

// retains `b` for the context's lifetime and makes sure its bytes are on the device; *rc keeps the first error
static crabml_hip_buf* hold(crabml_hip_llama* c, const crabml_hip_buf* b, int* rc) {
  crabml_hip_buf* m = const_cast<crabml_hip_buf*>(b);
  crabml_hip_buf_retain(m);
  c->held.push_back(m);
  if (*rc == 0) *rc = ensure_mem(c->dev, m);
  return m;
}

// the weights (every one is retained even behind an error: destroy releases what `held` lists), the activation table of the
// architecture, and the f16 prompt GEMM's A' range check of every matrix.  Returns the first error.
static int retain_weights(crabml_hip_llama* c, const crabml_hip_llama_weights_t* w, const crabml_hip_llama_arch_t* arch, const ModelFacts& f) {
  crabml_hip_device* dev = c->dev;
  const auto& g = c->cfg;
  int rc = 0;
  c->token_embed = hold(c, w->token_embed, &rc);
  c->rms_final = hold(c, w->rms_final_weight, &rc);
  c->output = hold(c, f.outw, &rc);
  for (size_t l = 0; l < g.n_layers; l++) {
    c->rms_att.push_back(hold(c, w->rms_att_weight[l], &rc));
    c->rms_ffn.push_back(hold(c, w->rms_ffn_weight[l], &rc));
    c->wq.push_back(hold(c, w->wq[l], &rc));
    c->wk.push_back(hold(c, w->wk[l], &rc));
    c->wv.push_back(hold(c, w->wv[l], &rc));
    c->wo.push_back(hold(c, w->wo[l], &rc));
    c->gate.push_back(hold(c, w->ffn_gate_weight[l], &rc));
    c->down.push_back(hold(c, w->ffn_down_weight[l], &rc));
    c->up.push_back(hold(c, w->ffn_up_weight[l], &rc));
    if (f.qwen2) {
      c->bq.push_back(hold(c, arch->bq[l], &rc));
      c->bk.push_back(hold(c, arch->bk[l], &rc));
      c->bv.push_back(hold(c, arch->bv[l], &rc));
    }
  }
  if (f.gemma) {  // (the table at create, not on the first gelu_inplace call: the step's graph is captured at create)
    if (rc == 0) rc = crabml_hip::ensure_gelu_table(dev);
    c->embed_scale = std::sqrt((float)g.embedding_dim);  // (embed_dim as f32).sqrt(), llama2.rs:468
    c->ffn_act = FfnAct{dev->gelu_table, 1};
  } else {
    c->ffn_act = FfnAct{dev->exp_table, 0};
  }
  // gemm_f16w_takes: one reduction over the scale plane, read back -- here once rather than inside the first prompt pass
  if (rc == 0 && !dev->strict_order && f.tp == 1 && (f.qt == CRABML_HIP_Q8_0 || f.qt == CRABML_HIP_Q8_1 || f.qt == CRABML_HIP_Q8_K))
    for (size_t l = 0; l < g.n_layers; l++)
      for (const crabml_hip_buf* m : {c->wq[l], c->wk[l], c->wv[l], c->wo[l], c->gate[l], c->up[l], c->down[l]})
        if (m->dtype != CRABML_HIP_Q5_K || (g.flags & CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM)) (void)gemm_f16w_takes(dev, m, f.qt);  // (Q5_K: opt-in)
  return rc;
}

// the KV caches (ours, or lazy.hip's runner's own: [n_kv_heads][seq_len][head_dim] in the configured element type, the layout of
// Llama2Runner's cache tensors, llama2.rs:65-86, used in place) and every buffer of the step, sized from the plan.  `rc`: the first
// error so far -- behind one nothing more is allocated; returns the first error.
static int alloc_step_buffers(crabml_hip_llama* c, crabml_hip_buf* const* ext_kc, crabml_hip_buf* const* ext_vc, int rc) {
  crabml_hip_device* dev = c->dev;
  const auto& g = c->cfg;
  const StepPlan& p = c->plan;
  const size_t dim = g.embedding_dim, dim_l = c->dim_l, kv_dim_l = c->kv_dim_l, hidden_l = c->hidden_l, n_kv_l = c->n_kv_l, n_heads_l = c->n_heads_l;
  auto A = [&](size_t bytes, auto** ptr) {
    if (rc == 0) rc = dalloc(c, bytes, (void**)ptr);
  };
  const size_t es = g.use_f16_kv_cache ? 2 : 4;
  c->kv_bytes = n_kv_l * g.seq_len * c->hd * es;
  c->kc.resize(g.n_layers);
  c->vc.resize(g.n_layers);
  for (size_t l = 0; l < g.n_layers; l++) {
    if (c->ext_kv) {
      const uint32_t kvt = g.use_f16_kv_cache ? CRABML_HIP_F16 : CRABML_HIP_F32;
      if (!ext_kc[l] || !ext_vc[l] || ext_kc[l]->dtype != kvt || ext_vc[l]->dtype != kvt || ext_kc[l]->n_elems * es != c->kv_bytes ||
          ext_vc[l]->n_elems * es != c->kv_bytes) {
        if (rc == 0) rc = set_error(dev, CRABML_HIP_BAD_INPUT, "llama: external kv cache of layer %zu has the wrong type or size", l);
        continue;
      }
      if (l == 0) c->ext_kc0 = ext_kc[l];
      c->kc[l] = hold(c, ext_kc[l], &rc)->ptr;
      c->vc[l] = hold(c, ext_vc[l], &rc)->ptr;
    } else {
      A(c->kv_bytes, &c->kc[l]);
      A(c->kv_bytes, &c->vc[l]);
    }
  }
  A(dim * 4, &c->x);
  A(dim * 4, &c->partial);
  A(dim_l * 4, &c->qbuf);
  A(dim_l * 4, &c->attn);
  A(hidden_l * 4, &c->h);
  A(g.vocab_size * 4, &c->logits);
  A(std::max({dim_l + 2 * kv_dim_l, 2 * hidden_l, dim}) * 4, &c->tmp);
  const auto act_bytes = [](uint32_t t, size_t n) { return t == CRABML_HIP_F32 ? (size_t)16 : act_layout(t, n).total; };
  A(std::max(act_bytes(c->qt, dim), act_bytes(c->out_qt, dim)), &c->act_dim);
  A(act_bytes(c->qt, dim_l), &c->act_attn);
  A(act_bytes(c->qt, hidden_l), &c->act_hid);
  A(dim * 4, &c->xn);
  A(g.seq_len * (size_t)(c->npairs ? c->npairs : 1) * 2 * 4, &c->rope);
  if (p.exact_long_ok) {
    A(n_heads_l * g.seq_len * 4, &c->scores_g);
    A(n_heads_l * g.seq_len * 2, &c->p16);
  }
  if (p.attn_flash) {
    A(n_kv_l * (size_t)p.flash_S * flash_part_floats((int)(n_heads_l / n_kv_l), c->hd) * 4, &c->flash_part);
    A(n_kv_l * 4, &c->flash_tick);
    if (rc == 0 && !dev->dry && hipMemsetAsync(c->flash_tick, 0, n_kv_l * 4, dev->stream) != hipSuccess) rc = CRABML_HIP_UNEXPECTED;
  }
  A(8 * sizeof(int), &c->state);
  A((dim / 16 + dim) * 8, &c->slots);
  if (p.defer_norm || p.k_norm_in) A(dim / 16 * 4, &c->rsums);
  if (p.q8k_producers) {
    A(dim_l * 8, &c->a8gran);
    A(hidden_l * 8, &c->h8gran);
  }
  c->out_cap = (int)g.seq_len;
  A((size_t)c->out_cap * 4, &c->out_tokens);
  A(ARGMAX_BLOCKS * 4, &c->am_val);
  A(ARGMAX_BLOCKS * 4, &c->am_idx);
  A(2 * sizeof(int), &c->am_best);
  return rc;
}

// RoPE table with the reference's own recurrence (rope.rs:47-54: theta_scale = 10000^(-2/hd), theta = pos,
// theta *= theta_scale per pair; base hard-coded) evaluated with the host libm, as the trait op does.
// Qwen2 and Gemma: NEOX's table (rope.rs:65-80: theta_i = pos / 10000^(2 i / hd), i < rope_dim / 2), the trait op's own code (lazy.hip)
static std::vector<float> rope_table(const crabml_hip_llama* c) {
  const size_t seq = c->cfg.seq_len, hd = (size_t)c->hd;
  std::vector<float> tab(seq * (size_t)(c->npairs ? c->npairs : 1) * 2, 0.f);
  const float theta_scale = powf(10000.0f, -2.0f / (float)hd);
  for (size_t p = 0; p < seq; p++) {
    if (c->qwen2 || c->gemma) {
      rope_table_neox(tab.data() + p * c->npairs * 2, p, hd, (size_t)c->npairs);
      continue;
    }
    float theta = (float)p;
    for (int i = 0; i < c->npairs; i++) {
      tab[(p * c->npairs + i) * 2] = cosf(theta);
      tab[(p * c->npairs + i) * 2 + 1] = sinf(theta);
      theta *= theta_scale;
    }
  }
  return tab;
}

// the rope table to the device, the step's state and hand-off words zeroed; blocks until done (`tab` is the caller's)
static hipError_t init_state(crabml_hip_llama* c, const std::vector<float>& tab) {
  const auto& g = c->cfg;
  hipStream_t st = c->dev->stream;
  hipError_t e = hipMemcpyAsync(c->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(c->state, 0, 8 * sizeof(int), st);
  // vocabulary split: the entries of the other ranks' shards read -inf (an element-wise max over the ranks is the all-gather)
  if (e == hipSuccess && c->split_vocab) e = hipMemsetD32Async((hipDeviceptr_t)c->logits, (int)0xff800000u, g.vocab_size, st);
  if (e == hipSuccess) e = hipMemsetAsync(c->slots, 0, (g.embedding_dim / 16 + g.embedding_dim) * 8, st);
  if (e == hipSuccess && c->a8gran) e = hipMemsetAsync(c->a8gran, 0, (size_t)c->dim_l * 8, st);
  if (e == hipSuccess && c->h8gran) e = hipMemsetAsync(c->h8gran, 0, (size_t)c->hidden_l * 8, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

// One decode step per attention variant into a graph (token / pos / step are read from device memory by the kernels).
// tp > 1 without a communicator = a rank of the single-device simulation: driven segment by segment, no graph.
// tp > 1 over RCCL launches eagerly unless CRABML_HIP_LLAMA_TP_GRAPH asks for the collectives to be captured too.
// False: the caller asked for the graph path on one device and it could not be had.
static bool capture_graphs(crabml_hip_llama* c, const ModelFacts& f) {
  const auto& g = c->cfg;
  const bool want_graph = !(g.flags & CRABML_HIP_LLAMA_NO_GRAPH) &&
                          (f.tp == 1 || f.tp_dry || f.p2p_comm || (c->comm != nullptr && (g.flags & CRABML_HIP_LLAMA_TP_GRAPH)));
  if (!want_graph) return true;
  const int nvar = c->plan.attn_long_ok ? (c->plan.flash_ticket_until > 0 ? 3 : 2) : 1;
  bool ok = true;
  for (int v = 0; v < nvar && ok; v++) ok = capture_step(c, v, &c->graph[v], &c->exec[v]);
  (void)hipGetLastError();
  c->use_graph = ok;
  c->attn_variant = 0;
  return ok || f.tp > 1;  // tp > 1: if RCCL could not be captured the step simply runs eagerly
}

// ext_kc / ext_vc (lazy.hip): the caller's KV caches, used in place (alloc_step_buffers)
static int llama_create_impl(crabml_hip_device_t* dev, const crabml_hip_llama_config_t* cfg, const crabml_hip_llama_weights_t* w,
                             crabml_hip_buf* const* ext_kc, crabml_hip_buf* const* ext_vc, crabml_hip_llama_t** out,
                             const crabml_hip_llama_arch_t* arch = nullptr) {
  if (!dev || !cfg || !w || !out) return CRABML_HIP_BAD_INPUT;
  *out = nullptr;
  ModelFacts f;
  CH_TRY(validate_config(dev, *cfg, w, arch, &f));
  CH_TRY(validate_weights(dev, *cfg, w, &f));
  if (!dev->dry) CH_USE(dev);
  const auto refuse = [&](const char* why) {
    return set_error(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama fused path: seq_len %zu is past the %zu positions of a one-workgroup score row (limit %zu): %s",
                     cfg->seq_len, (size_t)(K_ATTN_LDS / 4 - f.hd), MAX_SEQ_LEN, why);
  };
  if (const char* why = long_cache_refusal(*cfg, f, nullptr)) return refuse(why);
  const StepPlan plan = decide_step(dev, *cfg, f, read_flash_hooks());
  if (const char* why = long_cache_refusal(*cfg, f, &plan)) return refuse(why);
  crabml_hip_llama* c = nullptr;
  CH_TRY(new_context(dev, *cfg, f, plan, ext_kc != nullptr, &c));
  int rc = retain_weights(c, w, arch, f);
  rc = alloc_step_buffers(c, ext_kc, ext_vc, rc);
  if (rc != 0) {
    crabml_hip_llama_destroy(c);
    return rc;
  }
  const std::vector<float> tab = rope_table(c);
  if (dev->dry) {  // record-only test device: nothing to initialize, nothing to capture
    *out = c;
    return 0;
  }
  const hipError_t e = init_state(c, tab);
  if (e != hipSuccess) {
    crabml_hip_llama_destroy(c);
    return hip_fail(dev, e, "llama init", __FILE__, __LINE__);
  }
  if (!capture_graphs(c, f)) {  // fail loudly: the caller asked for the graph path
    crabml_hip_llama_destroy(c);
    CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: hipGraph capture/instantiate failed");
  }
  *out = c;
  return 0;
}

extern "C" {

int crabml_hip_llama_create(crabml_hip_device_t* dev, const crabml_hip_llama_config_t* cfg,
                            const crabml_hip_llama_weights_t* w, crabml_hip_llama_t** out) {
  if (!dev || !cfg || !w || !out) return CRABML_HIP_BAD_INPUT;
  *out = nullptr;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  return llama_create_impl(dev, cfg, w, nullptr, nullptr, out);
}

int crabml_hip_llama_create_arch(crabml_hip_device_t* dev, const crabml_hip_llama_config_t* cfg, const crabml_hip_llama_weights_t* w,
                                 const crabml_hip_llama_arch_t* arch, crabml_hip_llama_t** out) {
  if (!dev || !cfg || !w || !out) return CRABML_HIP_BAD_INPUT;
  *out = nullptr;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  return llama_create_impl(dev, cfg, w, nullptr, nullptr, out, arch);
}

int crabml_hip_llama_destroy(crabml_hip_llama_t* c) {
  if (!c) return 0;
  if (!c->dev->dry) {
    (void)hipSetDevice(c->dev->ordinal);
    (void)hipStreamSynchronize(c->dev->stream);
  }
  for (int v = 0; v < 3; v++) {
    if (c->exec[v]) (void)hipGraphExecDestroy(c->exec[v]);
    if (c->graph[v]) (void)hipGraphDestroy(c->graph[v]);
    if (c->sexec[v]) (void)hipGraphExecDestroy(c->sexec[v]);
    if (c->sgraph[v]) (void)hipGraphDestroy(c->sgraph[v]);
  }
  for (auto& a : c->allocs) pool_free(c->dev, a.first, a.second);
  for (auto* b : c->held) crabml_hip_buf_release(b);
  if (c->h_state) (void)hipHostFree(c->h_state);
  if (c->host_logits) (void)hipHostFree(c->host_logits);
  delete c;
  return 0;
}

static int check_step(crabml_hip_llama* c, size_t token, size_t pos) {
  crabml_hip_device* dev = c->dev;
  if (token >= c->cfg.vocab_size) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: token %zu out of range", token);
  if (pos != c->kv_len) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: pos %zu != kv cache length %zu", pos, c->kv_len);
  if (pos >= c->cfg.seq_len) CH_BAIL(dev, CRABML_HIP_TENSOR_ERROR, "llama: kv cache is full (%zu)", c->cfg.seq_len);
  return 0;
}

int crabml_hip_llama_forward(crabml_hip_llama_t* c, size_t token, size_t pos, float* logits) {
  if (!c) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = c->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  if (c->tp > 1 && !c->comm && !c->tp_dry)
    CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: a tp rank without a communicator is driven by crabml_hip_llama_tp_sim_*");
  CH_TRY(check_step(c, token, pos));
  CH_TRY(set_state(c, token, pos, 0));
  CH_TRY(run_step(c, pos));
  c->kv_len++;
  if (logits) {
    int fault = 0;
    CH_HIP(dev, hipMemcpyAsync(logits, c->logits, c->cfg.vocab_size * 4, hipMemcpyDeviceToHost, dev->stream));
    CH_HIP(dev, hipMemcpyAsync(&fault, c->state + 5, sizeof(int), hipMemcpyDeviceToHost, dev->stream));
    CH_HIP(dev, hipStreamSynchronize(dev->stream));
    if (fault == 2) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a tensor-parallel peer's partial sums never arrived (poll timed out)");
    if (fault) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a norm-epilogue gather timed out (workgroups not co-resident?)");
  }
  return 0;
}

int crabml_hip_llama_decode_greedy(crabml_hip_llama_t* c, size_t token, size_t n_steps, uint32_t* out_tokens) {
  if (!c || (!out_tokens && n_steps)) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = c->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  if (c->tp > 1 && !c->comm && !c->tp_dry)
    CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: a tp rank without a communicator is driven by crabml_hip_llama_tp_sim_*");
  if (token >= c->cfg.vocab_size) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: token %zu out of range", token);
  if (c->kv_len + n_steps > c->cfg.seq_len || n_steps > (size_t)c->out_cap)
    CH_BAIL(dev, CRABML_HIP_TENSOR_ERROR, "llama: %zu steps do not fit the kv cache (%zu of %zu used)", n_steps, c->kv_len, c->cfg.seq_len);
  if (n_steps == 0) return 0;
  CH_TRY(set_state(c, token, c->kv_len, 0));
  for (size_t s = 0; s < n_steps; s++) CH_TRY(run_step(c, c->kv_len + s));
  c->kv_len += n_steps;
  int fault = 0;
  CH_HIP(dev, hipMemcpyAsync(out_tokens, c->out_tokens, n_steps * 4, hipMemcpyDeviceToHost, dev->stream));
  CH_HIP(dev, hipMemcpyAsync(&fault, c->state + 5, sizeof(int), hipMemcpyDeviceToHost, dev->stream));
  CH_HIP(dev, hipStreamSynchronize(dev->stream));
  if (fault == 2) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a tensor-parallel peer's partial sums never arrived (poll timed out)");
  if (fault) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a norm-epilogue gather timed out (workgroups not co-resident?)");
  return 0;
}

int crabml_hip_llama_decode_sample(crabml_hip_llama_t* c, size_t token, size_t n_steps, float temperature, float topp, const float* coins,
                                   uint32_t* out_tokens) {
  if (!c || (!out_tokens && n_steps) || (!coins && n_steps)) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = c->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  if (c->tp > 1) CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama: decode_sample does not run on tensor-parallel ranks");
  if (std::isnan(temperature) || temperature < 0.f) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: temperature %g must be >= 0", (double)temperature);
  if (temperature == 0.0f) return crabml_hip_llama_decode_greedy(c, token, n_steps, out_tokens);  // sampler.rs:29-31
  if (!sample_args_ok(temperature, topp)) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: topp %g must be > 0", (double)topp);
  for (size_t s = 0; s < n_steps; s++)
    if (!(coins[s] >= 0.f && coins[s] < 1.f)) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: coin %zu = %g is not in [0, 1)", s, (double)coins[s]);
  if (c->ext_kv) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: a context of the recorded-op queue samples on the host");
  if (token >= c->cfg.vocab_size) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama: token %zu out of range", token);
  if (c->kv_len + n_steps > c->cfg.seq_len || n_steps > (size_t)c->out_cap)
    CH_BAIL(dev, CRABML_HIP_TENSOR_ERROR, "llama: %zu steps do not fit the kv cache (%zu of %zu used)", n_steps, c->kv_len, c->cfg.seq_len);
  if (n_steps == 0) return 0;
  CH_TRY(sample_alloc(c));
  const float par[2] = {temperature, topp};
  CH_TRY(stage_h2d(c, c->sm_par, par, sizeof par));
  CH_HIP(dev, hipMemcpyAsync(c->sm_coins, coins, n_steps * 4, hipMemcpyHostToDevice, dev->stream));
  CH_TRY(set_state(c, token, c->kv_len, 0));
  for (size_t s = 0; s < n_steps; s++) CH_TRY(run_step_sampled(c, c->kv_len + s));
  c->kv_len += n_steps;
  int fault = 0;
  CH_HIP(dev, hipMemcpyAsync(out_tokens, c->out_tokens, n_steps * 4, hipMemcpyDeviceToHost, dev->stream));
  CH_HIP(dev, hipMemcpyAsync(&fault, c->state + 5, sizeof(int), hipMemcpyDeviceToHost, dev->stream));
  CH_HIP(dev, hipStreamSynchronize(dev->stream));
  if (fault == SAMPLE_FAULT) {  // the context stays usable: the word is cleared, the caller sees the error
    CH_HIP(dev, hipMemsetAsync(c->state + 5, 0, sizeof(int), dev->stream));
    CH_HIP(dev, hipStreamSynchronize(dev->stream));
    CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: nothing to sample (the logits hold a NaN or +inf, or the nucleus is empty)");
  }
  if (fault == 2) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a tensor-parallel peer's partial sums never arrived (poll timed out)");
  if (fault) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a norm-epilogue gather timed out (workgroups not co-resident?)");
  return 0;
}

int crabml_hip_llama_prefill(crabml_hip_llama_t* c, const uint32_t* tokens, size_t n, float* logits) {
  if (!c || (!tokens && n)) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = c->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  CH_TRY(prefill_check(c, tokens, n));
  if (c->tp > 1) {  // token loop
    for (size_t i = 0; i < n; i++) CH_TRY(crabml_hip_llama_forward(c, tokens[i], c->kv_len, i + 1 == n ? logits : nullptr));
    return 0;
  }
  const size_t chunk = prefill_chunk_rows(c);
  CH_TRY(prefill_alloc(c, chunk));
  for (size_t i = 0; i < n; i += chunk) {
    const size_t B = n - i < chunk ? n - i : chunk;
    CH_TRY(prefill_chunk(c, tokens + i, B, c->kv_len, logits != nullptr && i + B == n));
    c->kv_len += B;
  }
  if (logits) {
    CH_HIP(dev, hipMemcpyAsync(logits, c->logits, c->cfg.vocab_size * 4, hipMemcpyDeviceToHost, dev->stream));
    CH_HIP(dev, hipStreamSynchronize(dev->stream));
  }
  return 0;
}

// Single-device simulation of a tensor-parallel group: `ranks[r]` was created with tp_size = n, tp_rank = r,
// tp_comm = NULL on the SAME device.  Segments are enqueued rank by rank and the all-reduce is a local kernel
// (sum in rank order).  Validates the sharding, the partial-sum plumbing and the residual hand-off on one GPU.
int crabml_hip_llama_tp_sim_forward(crabml_hip_llama_t* const* ranks, int n, size_t token, size_t pos, float* logits) {
  if (!ranks || n < 1 || n > 8 || !ranks[0]) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = ranks[0]->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  for (int r = 0; r < n; r++) {
    if (!ranks[r] || ranks[r]->dev != dev || ranks[r]->tp != n || ranks[r]->tp_rank != r || ranks[r]->comm)
      CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "tp_sim: rank %d is not a communicator-less rank %d of %d on this device", r, r, n);
    CH_TRY(check_step(ranks[r], token, pos));
    CH_TRY(set_state(ranks[r], token, pos, 0));
  }
  const int nseg = n_segments(ranks[0]);
  SimPtrs ptrs{};
  for (int r = 0; r < n; r++) ptrs.p[r] = ranks[r]->partial;
  const int dim = (int)ranks[0]->cfg.embedding_dim;
  for (int r = 0; r < n; r++) ranks[r]->attn_variant = variant_of(ranks[r], pos);
  for (int s = 0; s < nseg; s++) {
    for (int r = 0; r < n; r++) CH_TRY(enqueue_segment(ranks[r], s));
    if (n > 1 && s + 1 < nseg) k_sim_allreduce<<<(dim + 255) / 256, 256, 0, dev->stream>>>(ptrs, n, dim);
  }
  for (int r = 0; r < n; r++) ranks[r]->kv_len++;
  if (ranks[0]->split_vocab) {
    // every rank sampled from its own shard: the group's token is the rank-order combination of the pairs
    SimBest sb{};
    for (int r = 0; r < n; r++) {
      if (!ranks[r]->split_vocab) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "tp_sim: rank %d does not split the vocabulary like rank 0", r);
      sb.best[r] = ranks[r]->am_best;
      sb.token[r] = ranks[r]->state;
      sb.step[r] = ranks[r]->state + 2;
      sb.out_tokens[r] = ranks[r]->out_tokens;
    }
    k_sim_argmax_combine<<<1, 64, 0, dev->stream>>>(sb, n, ranks[0]->out_cap);
    CH_HIP(dev, hipGetLastError());
  }
  if (logits) {
    if (ranks[0]->split_vocab) {
      for (int r = 0; r < n; r++)
        CH_HIP(dev, hipMemcpyAsync(logits + ranks[r]->vocab_off, ranks[r]->logits + ranks[r]->vocab_off, (size_t)ranks[r]->vocab_l * 4,
                                   hipMemcpyDeviceToHost, dev->stream));
    } else {
      CH_HIP(dev, hipMemcpyAsync(logits, ranks[0]->logits, ranks[0]->cfg.vocab_size * 4, hipMemcpyDeviceToHost, dev->stream));
    }
    CH_HIP(dev, hipStreamSynchronize(dev->stream));
  }
  return 0;
}

size_t crabml_hip_llama_kv_len(const crabml_hip_llama_t* c) { return c ? c->kv_len : 0; }

int crabml_hip_llama_reset(crabml_hip_llama_t* c) {
  if (!c) return CRABML_HIP_BAD_INPUT;
  c->kv_len = 0;
  if (c->flash_tick) {  // a step that faulted half-way may have left arrivals behind
    CH_USE(c->dev);
    CH_FLUSH(c->dev);
    CH_HIP(c->dev, hipMemsetAsync(c->flash_tick, 0, (size_t)c->n_kv_l * 4, c->dev->stream));
  }
  return 0;
}

int crabml_hip_llama_debug_kv(crabml_hip_llama_t* c, size_t layer, int32_t which_v, void* dst, size_t nbytes) {
  if (!c || !dst) return CRABML_HIP_BAD_INPUT;
  CH_USE(c->dev);
  CH_FLUSH(c->dev);
  if (layer >= c->cfg.n_layers || nbytes > c->kv_bytes) CH_BAIL(c->dev, CRABML_HIP_BAD_INPUT, "llama debug_kv: bad layer/size");
  CH_HIP(c->dev, hipMemcpyAsync(dst, which_v ? c->vc[layer] : c->kc[layer], nbytes, hipMemcpyDeviceToHost, c->dev->stream));
  CH_HIP(c->dev, hipStreamSynchronize(c->dev->stream));
  return 0;
}

// test hook (crabml_hip_debug.h, where the classes are listed): the cache rows past kv_len, the step's data scratch and the prompt
// pass's row buffers filled with a pattern, in stream order.  A buffer is filled as the whole pool block dalloc gave it.
int crabml_hip_llama_debug_poison(crabml_hip_llama_t* c, uint32_t what, uint16_t fill16, uint32_t fill32) {
  if (!c || (what & ~7u)) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = c->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  if (c->tp > 1 || c->ext_kv)
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED, "llama debug_poison: one device and the context's own KV cache only");
  hipStream_t st = dev->stream;
  auto words = [&](void* p, size_t bytes, bool half) -> int {
    if (half)
      CH_HIP(dev, hipMemsetD16Async((hipDeviceptr_t)p, fill16, bytes / 2, st));
    else
      CH_HIP(dev, hipMemsetD32Async((hipDeviceptr_t)p, (int)fill32, bytes / 4, st));
    return 0;
  };
  auto fill = [&](void* p, bool half) -> int {
    if (!p) return 0;
    for (const auto& a : c->allocs)
      if (a.first == p) return words(p, a.second, half);
    CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama debug_poison: a buffer that is no allocation of the context");
  };
  if (what & 1) {
    const auto& g = c->cfg;
    const bool kv16 = g.use_f16_kv_cache != 0;
    const size_t es = kv16 ? 2 : 4, hd = (size_t)c->hd, live = c->kv_len < g.seq_len ? c->kv_len : g.seq_len;
    const size_t tail = (g.seq_len - live) * hd * es;
    for (size_t l = 0; l < g.n_layers && tail; l++)
      for (void* base : {c->kc[l], c->vc[l]})
        for (size_t h = 0; h < (size_t)c->n_kv_l; h++) CH_TRY(words((char*)base + (h * g.seq_len + live) * hd * es, tail, kv16));
  }
  if (what & 2) {
    for (void* p : {(void*)c->x, (void*)c->partial, (void*)c->qbuf, (void*)c->attn, (void*)c->h, (void*)c->tmp, (void*)c->xn, (void*)c->logits,
                    (void*)c->rsums, (void*)c->scores_g, (void*)c->flash_part, (void*)c->am_val, (void*)c->out_tokens})
      CH_TRY(fill(p, false));
    for (void* p : {(void*)c->act_dim, (void*)c->act_attn, (void*)c->act_hid, (void*)c->p16}) CH_TRY(fill(p, true));
  }
  if ((what & 4) && c->pf_cap) {
    for (void* p : {(void*)c->pf_x, (void*)c->pf_xn, (void*)c->pf_q, (void*)c->pf_k, (void*)c->pf_v, (void*)c->pf_qr, (void*)c->pf_attn,
                    (void*)c->pf_tmp, (void*)c->pf_g, (void*)c->pf_u, (void*)c->pf_split, (void*)c->pf_scores})
      CH_TRY(fill(p, false));
    for (void* p : {(void*)c->pf_act_dim, (void*)c->pf_act_hid, c->pf_xh, c->pf_xh2, (void*)c->pf_p16}) CH_TRY(fill(p, true));
  }
  return 0;
}

// parity hook (crabml_hip_debug.h): one eager decode step with the buffers of one layer copied out between its launches
int crabml_hip_llama_debug_tap(crabml_hip_llama_t* c, size_t token, size_t pos, size_t layer, float* logits, void* dst, size_t dst_bytes,
                               crabml_hip_tap_entry_t* dir, size_t* need) {
  if (!c || (dst && !dir) || (!dst && !need)) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = c->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  // (decide_step: what Fused5 / FusedK and !ordered imply)
  if ((c->plan.path != SegPath::Fused5 && c->plan.path != SegPath::FusedK) || c->plan.ordered || c->tp > 1 || c->ext_kv)
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED,
            "llama debug_tap: only the fused launches of the fast step (Q4_0 / Q8_0 / Q4_1 / Q5_0 / Q5_1 layers, a K-quant body and the mixes it takes: KBodies) on one device with its own KV cache");
  if (layer >= c->cfg.n_layers) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama debug_tap: layer %zu of %zu", layer, (size_t)c->cfg.n_layers);
  const size_t dim = c->cfg.embedding_dim, hidden = c->cfg.hidden_dim;
  // the row type of every field that leaves as blocks (the others: f32 values, the plan words)
  const uint32_t qt = c->qt, cq = c->out_qt;
  TapField fld[CRABML_HIP_TAP_FIELDS];
  fld[CRABML_HIP_TAP_QKV_IN_ACT] = fld[CRABML_HIP_TAP_WO_ACT] = fld[CRABML_HIP_TAP_DOWN_ACT] = fld[CRABML_HIP_TAP_ACT_ATTN] = TapField{qt, dim};
  fld[CRABML_HIP_TAP_ACT_HID] = TapField{qt, hidden};
  if (cq == CRABML_HIP_Q8_0 || cq == CRABML_HIP_Q8_1 || cq == CRABML_HIP_Q8_K) fld[CRABML_HIP_TAP_CLS_ACT] = TapField{cq, dim};
  for (int f : {CRABML_HIP_TAP_QKV_IN_QP, CRABML_HIP_TAP_ACT_ATTN_QP, CRABML_HIP_TAP_WO_QP, CRABML_HIP_TAP_ACT_HID_QP, CRABML_HIP_TAP_DOWN_QP,
                CRABML_HIP_TAP_CLS_QP})
    fld[f] = TapField{CRABML_HIP_Q8_K, 0};  // raw bytes: one per element, class-major inside every 32-group
  const size_t cls_raw = fld[CRABML_HIP_TAP_CLS_ACT].cols ? act_layout(cq, dim).total : dim * 4;
  // the scratch area, in the device's plane layout (every term a multiple of 256, the fields' alignment): three x, qbuf, attn and the
  // three xn of the K-quant path (one to spare); h; the four dim-long plane sets (in front of q|k|v, act_attn, behind wo, behind
  // ffn_down), act_hid, the classifier's; three rsums of up to two sums per chunk; the class-major planes of those five dim-long sets
  // and of act_hid
  const size_t adb = act_layout(qt, dim).total, ahb = act_layout(qt, hidden).total;
  const size_t raw_cap = 9 * align_up(dim * 4, 256) + align_up(hidden * 4, 256) + 4 * adb + 3 * align_up(dim / 16 * 4, 256) + ahb +
                         align_up(cls_raw, 256) + 5 * align_up(dim, 256) + align_up(hidden, 256) + 512;
  if (need) *need = raw_cap;
  if (!dst) return 0;
  if (dst_bytes < raw_cap) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama debug_tap: dst holds %zu bytes, %zu needed", dst_bytes, raw_cap);
  CH_TRY(check_step(c, token, pos));
  TapRec& tap = c->tap;
  CH_TRY(tap.ensure(c, raw_cap));
  CH_TRY(set_state(c, token, pos, 0));
  // the eager step (run_step without the graph replay)
  c->attn_variant = variant_of(c, pos);
  tap.arm((int)layer);
  tap.note(CRABML_HIP_PLAN_N_CU, dev->n_cu);
  tap.note(CRABML_HIP_PLAN_DEFER_NORM, c->plan.defer_norm ? 1 : 0);
  tap.note(CRABML_HIP_PLAN_NORM_EPILOGUE, c->plan.norm_epi ? 1 : 0);
  tap.note(CRABML_HIP_PLAN_ATTN_VARIANT, c->attn_variant + (c->attn_variant >= 1 && c->plan.attn_flash ? 16 : 0));
  tap.note(CRABML_HIP_PLAN_PATH, (int32_t)c->plan.path);
  tap.note(CRABML_HIP_PLAN_NORM_EPI_K, c->plan.norm_epi_k ? 1 : 0);
  tap.note(CRABML_HIP_PLAN_Q8K_PRODUCERS, c->plan.q8k_producers ? 1 : 0);
  tap.note(CRABML_HIP_PLAN_K_NORM_IN, c->plan.k_norm_in ? 1 : 0);
  const int rc = enqueue_step(c);
  tap.disarm();
  if (rc != 0) return rc;
  c->kv_len++;
  std::vector<uint8_t> h;
  int fault = 0;
  if (logits) CH_HIP(dev, hipMemcpyAsync(logits, c->logits, c->cfg.vocab_size * 4, hipMemcpyDeviceToHost, dev->stream));
  CH_HIP(dev, hipMemcpyAsync(&fault, c->state + 5, sizeof(int), hipMemcpyDeviceToHost, dev->stream));
  CH_TRY(tap.read_back(dev, &h));
  CH_HIP(dev, hipStreamSynchronize(dev->stream));
  if (fault) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "llama: a norm-epilogue gather timed out (workgroups not co-resident?)");
  return export_fields(dev, tap, h, fld, CRABML_HIP_TAP_FIELDS, CRABML_HIP_TAP_PLAN, CRABML_HIP_TAP_PLAN_WORDS, dst, dst_bytes, dir);
}

// parity hook (crabml_hip_debug.h): one chunk pass of the prompt path with the row buffers of one layer copied out between its launches
int crabml_hip_llama_debug_prefill_tap(crabml_hip_llama_t* c, const uint32_t* tokens, size_t n, size_t layer, float* logits, void* dst,
                                       size_t dst_bytes, crabml_hip_tap_entry_t* dir, size_t* need) {
  if (!c || (!tokens && n) || (dst && !dir) || (!dst && !need)) return CRABML_HIP_BAD_INPUT;
  crabml_hip_device* dev = c->dev;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  const bool rows_8 = (c->qt == CRABML_HIP_Q8_0 || c->qt == CRABML_HIP_Q8_1) &&
                      (c->wtype == CRABML_HIP_Q4_0 || c->wtype == CRABML_HIP_Q8_0 || c->wtype == CRABML_HIP_Q4_1 || c->wtype == CRABML_HIP_Q5_0 ||
                       c->wtype == CRABML_HIP_Q5_1);  // (Q5_0 / Q5_1: the same Q8_0 / Q8_1 row fields and plan words; tests/test_hip_prefill_q5_01_launches.py)
  // Q8_K rows: every layer matrix Q4_K, Q5_K or Q6_K (the *_K_M mixes), the classifier one of them too; a context created with
  // CRABML_HIP_LLAMA_PREFILL_TAP_Q2K_Q3K: Q2_K and Q3_K matrices as well (the Q2_K / Q3_K recipes)
  bool rows_k = c->qt == CRABML_HIP_Q8_K;
  const bool q23 = (c->cfg.flags & CRABML_HIP_LLAMA_PREFILL_TAP_Q2K_Q3K) != 0;
  auto k_body = [q23](const crabml_hip_buf* w) {
    return w->dtype == CRABML_HIP_Q4_K || w->dtype == CRABML_HIP_Q5_K || w->dtype == CRABML_HIP_Q6_K ||
           (q23 && (w->dtype == CRABML_HIP_Q2_K || w->dtype == CRABML_HIP_Q3_K));
  };
  for (size_t l = 0; rows_k && l < c->cfg.n_layers; l++)
    for (const crabml_hip_buf* w : {c->wq[l], c->wk[l], c->wv[l], c->wo[l], c->gate[l], c->up[l], c->down[l]}) rows_k = rows_k && k_body(w);
  rows_k = rows_k && k_body(c->output);
  if (c->tp > 1 || dev->strict_order || c->ext_kv || !(rows_8 || rows_k))
    CH_BAIL(dev, CRABML_HIP_NOT_IMPLEMENTED,
            "llama debug_prefill_tap: only Q4_0 / Q8_0 / Q4_1 / Q5_0 / Q5_1 and Q4_K / Q5_K / Q6_K layers (the *_K_M mixes; Q2_K / Q3_K: PREFILL_TAP_Q2K_Q3K) of the fast prompt pass on one device");
  if (layer >= c->cfg.n_layers) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama debug_prefill_tap: layer %zu of %zu", layer, (size_t)c->cfg.n_layers);
  CH_TRY(prefill_check(c, tokens, n));
  const size_t chunk = prefill_chunk_rows(c);
  if (n > chunk) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama debug_prefill_tap: %zu rows, one chunk pass holds %zu", n, chunk);
  const size_t dim = c->cfg.embedding_dim, hidden = c->cfg.hidden_dim, kv_dim = (size_t)c->kv_dim_l;
  const uint32_t qt = c->qt, cq = c->out_qt;
  const bool cls_q = cq == CRABML_HIP_Q8_0 || cq == CRABML_HIP_Q8_1 || cq == CRABML_HIP_Q8_K;
  TapField fld[CRABML_HIP_PFTAP_FIELDS];  // (every field holds the n rows of the pass; the classifier's input is the last row's)
  fld[CRABML_HIP_PFTAP_N1_ACT] = fld[CRABML_HIP_PFTAP_ATTN_ACT] = fld[CRABML_HIP_PFTAP_N2_ACT] = TapField{qt, dim, n};
  fld[CRABML_HIP_PFTAP_HID_ACT] = TapField{qt, hidden, n};
  for (int f : {CRABML_HIP_PFTAP_N1_XH, CRABML_HIP_PFTAP_ATTN_XH, CRABML_HIP_PFTAP_N2_XH, CRABML_HIP_PFTAP_HID_XH}) fld[f].qtype = CRABML_HIP_F16;
  if (cls_q) fld[CRABML_HIP_PFTAP_CLS_ACT] = TapField{cq, dim, 1};
  if (qt == CRABML_HIP_Q8_K) {
    fld[CRABML_HIP_PFTAP_N1_QP] = TapField{CRABML_HIP_Q8_K, dim, n, CRABML_HIP_PFTAP_N1_ACT};
    fld[CRABML_HIP_PFTAP_ATTN_QP] = TapField{CRABML_HIP_Q8_K, dim, n, CRABML_HIP_PFTAP_ATTN_ACT};
    fld[CRABML_HIP_PFTAP_N2_QP] = TapField{CRABML_HIP_Q8_K, dim, n, CRABML_HIP_PFTAP_N2_ACT};
    fld[CRABML_HIP_PFTAP_HID_QP] = TapField{CRABML_HIP_Q8_K, hidden, n, CRABML_HIP_PFTAP_HID_ACT};
  }
  if (cq == CRABML_HIP_Q8_K) fld[CRABML_HIP_PFTAP_CLS_QP] = TapField{CRABML_HIP_Q8_K, dim, 1, CRABML_HIP_PFTAP_CLS_ACT};
  fld[CRABML_HIP_PFTAP_N1_XH_V].qtype = CRABML_HIP_F16;
  // the scratch area, in the device's layout: twelve (n, dim) f32 buffers (the two f32 norms among them), three sets of up to 7 k
  // pieces, k and v, g, u and h, three sets of act_dim planes and one of act_hid, their f16 planes (v's own among them), the last row,
  // the final norm's row and the classifier's input; every field 256-aligned.  The class-major planes are part of the Q8_K planes in
  // the area (a row's blocks and its class-major plane together are never larger than its planes: dst needs no more for them)
  const size_t adb = act_layout(qt, dim).total, ahb = act_layout(qt, hidden).total;
  const size_t cls_raw = cls_q ? act_layout(cq, dim).total : dim * 4;
  const size_t raw_cap = (12 + 21) * n * dim * 4 + 2 * n * kv_dim * 4 + 3 * n * hidden * 4 + 3 * n * adb + n * ahb + 4 * n * dim * 2 +
                         n * hidden * 2 + 2 * dim * 4 + cls_raw + 256 * (size_t)CRABML_HIP_PFTAP_FIELDS +
                         CRABML_HIP_PFTAP_PLAN_WORDS * sizeof(int32_t);
  if (need) *need = raw_cap;
  if (!dst) return 0;
  if (dst_bytes < raw_cap) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "llama debug_prefill_tap: dst holds %zu bytes, %zu needed", dst_bytes, raw_cap);
  CH_TRY(prefill_alloc(c, chunk));
  CH_TRY(c->pftap.ensure(c, raw_cap));
  CH_TRY(prefill_chunk(c, tokens, n, c->kv_len, true, (int)layer));
  c->kv_len += n;
  std::vector<uint8_t> h;
  if (logits) CH_HIP(dev, hipMemcpyAsync(logits, c->logits, c->cfg.vocab_size * 4, hipMemcpyDeviceToHost, dev->stream));
  CH_TRY(c->pftap.read_back(dev, &h));
  CH_HIP(dev, hipStreamSynchronize(dev->stream));
  return export_fields(dev, c->pftap, h, fld, CRABML_HIP_PFTAP_FIELDS, CRABML_HIP_PFTAP_PLAN, CRABML_HIP_PFTAP_PLAN_WORDS, dst, dst_bytes, dir);
}

// test hook (crabml_hip_debug.h): the step plan of the context this configuration creates; the record-only device is welcome
int crabml_hip_debug_step_plan(crabml_hip_device_t* dev, const crabml_hip_llama_config_t* cfg, const crabml_hip_llama_weights_t* w,
                               const crabml_hip_llama_arch_t* arch, int32_t* words, size_t n_words) {
  if (!dev || !cfg || !w || !words || n_words < CRABML_HIP_STEPPLAN_WORDS) return CRABML_HIP_BAD_INPUT;
  if (!dev->dry) CH_USE(dev);
  CH_FLUSH(dev);
  crabml_hip_llama* c = nullptr;
  CH_TRY(llama_create_impl(dev, cfg, w, nullptr, nullptr, &c, arch));
  const StepPlan& p = c->plan;
  int graphs = 0;
  for (int v = 0; v < 3; v++) graphs += c->exec[v] != nullptr;
  const int32_t v[CRABML_HIP_STEPPLAN_WORDS] = {
      (int32_t)p.path, p.ordered, p.norm_epi, p.norm_epi_k, p.defer_norm, p.gu_rows, p.q8k_producers, p.k_norm_in, p.attn_long_ok,
      p.exact_long_ok, (int32_t)p.attn_long_from, p.pv_split, p.attn_flash, p.flash_ticket, (int32_t)p.flash_ticket_until, p.attn_flash_rows,
      p.flash_S, p.flash_min_rows, p.attn_s_rows, (int32_t)p.attn_s_lds, c->use_graph, graphs, dev->n_cu};  // CRABML_HIP_STEPPLAN_* order
  memcpy(words, v, sizeof v);
  (void)crabml_hip_llama_destroy(c);
  return 0;
}

// parity hook (crabml_hip_debug.h): k_attn_flash by itself, on caller-supplied q / K / V
int crabml_hip_debug_sample(crabml_hip_device_t* dev, const float* logits, size_t n, float temperature, float topp, float coin,
                            uint32_t* token) {
  if (!dev || !logits || !token || n == 0 || n > ((size_t)1 << 24)) return CRABML_HIP_BAD_INPUT;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  if (std::isnan(temperature) || temperature < 0.f) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "debug_sample: temperature %g must be >= 0", (double)temperature);
  const bool greedy = temperature == 0.0f;
  if (!greedy && !sample_args_ok(temperature, topp)) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "debug_sample: topp %g must be > 0", (double)topp);
  if (!greedy && !(coin >= 0.f && coin < 1.f)) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "debug_sample: coin %g is not in [0, 1)", (double)coin);
  const size_t o_x = 0, o_keys = align_up(n * 4, 256), o_hist = align_up(o_keys + n * 2, 256), o_bmax = align_up(o_hist + SAMPLE_HIST * 4, 256),
               o_par = o_bmax + 1024, o_coin = o_par + 256, o_state = o_coin + 256, o_out = o_state + 256, o_amv = o_out + 256,
               o_ami = o_amv + ARGMAX_BLOCKS * 4, total = o_ami + ARGMAX_BLOCKS * 4;
  char* base = nullptr;
  CH_HIP(dev, hipMalloc((void**)&base, total));
  hipStream_t st = dev->stream;
  const float par[2] = {temperature, topp};
  int* state = (int*)(base + o_state);
  unsigned* outp = (unsigned*)(base + o_out);
  int fault = 0;
  uint32_t tok = 0;
  hipError_t e = hipMemsetAsync(base + o_hist, 0, SAMPLE_HIST * 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(state, 0, 256, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_x, logits, n * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_par, par, sizeof par, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_coin, &coin, 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const float* x = (const float*)(base + o_x);
    if (greedy) {
      k_argmax_partial<<<ARGMAX_BLOCKS, 256, 0, st>>>(x, (int)n, (float*)(base + o_amv), (int*)(base + o_ami), 0);
      k_argmax_step<<<1, 64, 0, st>>>((const float*)(base + o_amv), (const int*)(base + o_ami), ARGMAX_BLOCKS, state, state + 1, state + 2, outp, 1,
                                      state + 4, (int*)nullptr);
    } else {
      const SampleStep ss{(const float*)(base + o_par), (const float*)(base + o_coin), state, state + 1, state + 2, state + 4, outp, 1, state + 5};
      unsigned short* keys = (unsigned short*)(base + o_keys);
      unsigned* hist = (unsigned*)(base + o_hist);
      k_sample_max<<<SAMPLE_BLOCKS, 256, 0, st>>>(x, (int)n, ss.par, (float*)(base + o_bmax));
      k_sample_keys<<<SAMPLE_BLOCKS, 256, 0, st>>>(x, (int)n, ss.par, (const float*)(base + o_bmax), SAMPLE_BLOCKS,
                                                   (const unsigned short*)dev->exp_table, keys, hist);
      if (dev->strict_order)
        k_sample_pick<true><<<1, SAMPLE_PICK_THREADS, 0, st>>>(keys, (int)n, hist, ss);
      else
        k_sample_pick<false><<<1, SAMPLE_PICK_THREADS, 0, st>>>(keys, (int)n, hist, ss);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&tok, outp, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&fault, state + 5, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(base);
  if (e != hipSuccess) return hip_fail(dev, e, "debug_sample", __FILE__, __LINE__);
  if (fault) CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "debug_sample: nothing to sample (the logits hold a NaN or +inf, or the nucleus is empty)");
  *token = tok;
  return 0;
}

int crabml_hip_debug_flash_attention(crabml_hip_device_t* dev, const float* q, const uint16_t* k, const uint16_t* v, size_t n_heads,
                                     size_t n_kv, size_t head_dim, size_t seq, size_t seq_cap, size_t slices, float* out, float* out2) {
  if (!dev || !q || !k || !v || !out || seq == 0 || seq_cap < seq || n_kv == 0 || n_heads % n_kv != 0) return CRABML_HIP_BAD_INPUT;
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  const int grp = (int)(n_heads / n_kv), hd = (int)head_dim;
  const FlashFn fn = flash_kernel(grp, hd, false, false), fnt = flash_kernel(grp, hd, false, true);
  const bool ticket_form = out2 != nullptr;
  if (fn == nullptr || slices < 1 || slices > FLASH_MAX_SLICES) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "debug_flash_attention: unsupported group / head_dim / slices");
  if (raise_dyn_lds(dev, (const void*)fn, (int)flash_lds_bytes(grp, hd)) != hipSuccess ||
      raise_dyn_lds(dev, (const void*)fnt, (int)flash_lds_bytes(grp, hd)) != hipSuccess)
    CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "debug_flash_attention: LDS");
  const size_t nq = n_heads * head_dim * 4, nkv = n_kv * seq_cap * head_dim * 2, npart = n_kv * slices * flash_part_floats(grp, hd) * 4;
  char* base = nullptr;
  const size_t o_q = 0, o_k = align_up(o_q + nq, 256), o_v = align_up(o_k + nkv, 256), o_out = align_up(o_v + nkv, 256),
               o_part = align_up(o_out + nq, 256), o_tick = align_up(o_part + npart, 256), o_pos = o_tick + align_up(n_kv * 4, 256),
               total = o_pos + 256;
  CH_HIP(dev, hipMalloc((void**)&base, total));
  hipStream_t st = dev->stream;
  const int pos = (int)seq - 1;
  hipError_t e = hipMemsetAsync(base + o_tick, 0, n_kv * 4, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_q, q, nq, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_k, k, nkv, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_v, v, nkv, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_pos, &pos, 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (`pos` leaves scope)
  if (e == hipSuccess) {
    // the shipped form first (partials, then the merge launch), then the single-launch form (last arriver merges) twice on the
    // same ticket words -- the second launch finds them re-armed by the first; all three write the same `out`
    hipLaunchKernelGGL(fn, dim3((unsigned)(n_kv * slices)), dim3(flash_threads(grp)), (uint32_t)flash_lds_bytes(grp, hd), st,
                       (const float*)(base + o_q), (const unsigned short*)(base + o_k), (const unsigned short*)(base + o_v),
                       (const int*)(base + o_pos), (float*)(base + o_part), (unsigned*)(base + o_tick), (float*)(base + o_out),
                       (signed char*)nullptr, (unsigned short*)nullptr, (void*)nullptr, (int)seq_cap, (int)slices, FLASH_MIN_ROWS);
    with_const_else<256, 128, 64>(hd, [&](auto hdc) {  // (flash_kernel has no other head_dim)
      constexpr int HD = decltype(hdc)::value;
      hipLaunchKernelGGL((k_attn_flash_merge<HD, false>), dim3((unsigned)n_heads), dim3(HD), 0, st, (const float*)(base + o_part),
                         (const int*)(base + o_pos), (float*)(base + o_out), (signed char*)nullptr, (unsigned short*)nullptr, (void*)nullptr, grp,
                         (int)slices, FLASH_MIN_ROWS);
    });
    if (ticket_form) {
      e = hipMemcpyAsync(out2, base + o_out, nq, hipMemcpyDeviceToHost, st);  // (stream order: before the next launches overwrite it)
      for (int rep = 0; rep < 2 && e == hipSuccess; rep++)
        hipLaunchKernelGGL(fnt, dim3((unsigned)(n_kv * slices)), dim3(flash_threads(grp)), (uint32_t)flash_lds_bytes(grp, hd), st,
                           (const float*)(base + o_q), (const unsigned short*)(base + o_k), (const unsigned short*)(base + o_v),
                           (const int*)(base + o_pos), (float*)(base + o_part), (unsigned*)(base + o_tick), (float*)(base + o_out),
                           (signed char*)nullptr, (unsigned short*)nullptr, (void*)nullptr, (int)seq_cap, (int)slices, FLASH_MIN_ROWS);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, base + o_out, nq, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(base);
  if (e != hipSuccess) return hip_fail(dev, e, "debug_flash_attention", __FILE__, __LINE__);
  return 0;
}

// parity hook (crabml_hip_debug.h): the fast prompt pass's causal attention kernel by itself
int crabml_hip_debug_flash_attention_rows(crabml_hip_device_t* dev, const float* q, const uint16_t* k, const uint16_t* v, size_t n_heads,
                                          size_t n_kv, size_t head_dim, size_t pos0, size_t rows, size_t seq_cap, float* out) {
  if (!dev || !q || !k || !v || !out || rows == 0 || n_kv == 0 || n_heads % n_kv != 0 || seq_cap < pos0 + rows) return CRABML_HIP_BAD_INPUT;
  if (head_dim != 128 && head_dim != 64) CH_BAIL(dev, CRABML_HIP_BAD_INPUT, "debug_flash_attention_rows: head_dim 64 / 128");
  CH_LIVE(dev);
  CH_USE(dev);
  CH_FLUSH(dev);
  const FlashRowsFn fn = flash_rows_kernel((int)head_dim);
  if (raise_dyn_lds(dev, (const void*)fn, (int)flash_rows_lds_bytes((int)head_dim)) != hipSuccess)
    CH_BAIL(dev, CRABML_HIP_UNEXPECTED, "debug_flash_attention_rows: LDS");
  const size_t seq = seq_cap;
  const size_t nq = rows * n_heads * head_dim * 4, nkv = n_kv * seq * head_dim * 2;
  const size_t o_q = 0, o_k = align_up(o_q + nq, 256), o_v = align_up(o_k + nkv, 256), o_out = align_up(o_v + nkv, 256),
               o_pos = align_up(o_out + nq, 256), total = o_pos + 256;
  char* base = nullptr;
  CH_HIP(dev, hipMalloc((void**)&base, total));
  hipStream_t st = dev->stream;
  const int p0 = (int)pos0;
  hipError_t e = hipMemcpyAsync(base + o_q, q, nq, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_k, k, nkv, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_v, v, nkv, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + o_pos, &p0, 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) {
    const dim3 fg((unsigned)((rows + 63) / 64), (unsigned)n_heads);
    fn<<<fg, 512, flash_rows_lds_bytes((int)head_dim), st>>>((const float*)(base + o_q), (const unsigned short*)(base + o_k), (const unsigned short*)(base + o_v),
                                                             (const int*)(base + o_pos), (float*)(base + o_out), (int)n_heads, (int)n_kv, (int)seq, (int)rows);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, base + o_out, nq, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(base);
  if (e != hipSuccess) return hip_fail(dev, e, "debug_flash_attention_rows", __FILE__, __LINE__);
  return 0;
}

}  // extern "C"

// ==============================================================================================================
// The decode context as lazy.hip drives it: built from the buffers a recorded token of the reference's unchanged runner
// names (its weight handles, its own KV caches), stepped one SEGMENT at a time while the host is still recording the
// next one.  Everything below runs the same enqueue_segment as crabml_hip_llama_forward.
// ==============================================================================================================
namespace crabml_hip {

int lazy_ctx_create(crabml_hip_device* dev, const LazyModel& m, crabml_hip_llama** out) {
  *out = nullptr;
  crabml_hip_llama_weights_t w{};
  w.token_embed = m.token_embed;
  w.rms_att_weight = m.rms_att.data();
  w.rms_ffn_weight = m.rms_ffn.data();
  w.wq = m.wq.data();
  w.wk = m.wk.data();
  w.wv = m.wv.data();
  w.wo = m.wo.data();
  w.ffn_gate_weight = m.gate.data();
  w.ffn_down_weight = m.down.data();
  w.ffn_up_weight = m.up.data();
  w.rms_final_weight = m.rms_final;
  w.output_weight = m.output;
  const size_t L = m.cfg.n_layers;
  if (m.rms_att.size() != L || m.rms_ffn.size() != L || m.wq.size() != L || m.wk.size() != L || m.wv.size() != L || m.wo.size() != L ||
      m.gate.size() != L || m.down.size() != L || m.up.size() != L || m.kc.size() != L || m.vc.size() != L)
    return CRABML_HIP_BAD_INPUT;
  if (m.arch == CRABML_HIP_ARCH_LLAMA) return llama_create_impl(dev, &m.cfg, &w, m.kc.data(), m.vc.data(), out);
  if (m.arch == CRABML_HIP_ARCH_GEMMA) {
    const crabml_hip_llama_arch_t arch{CRABML_HIP_ARCH_GEMMA, nullptr, nullptr, nullptr};
    return llama_create_impl(dev, &m.cfg, &w, m.kc.data(), m.vc.data(), out, &arch);
  }
  if (m.bq.size() != L || m.bk.size() != L || m.bv.size() != L) return CRABML_HIP_BAD_INPUT;
  const crabml_hip_llama_arch_t arch{CRABML_HIP_ARCH_QWEN2, m.bq.data(), m.bk.data(), m.bv.data()};
  return llama_create_impl(dev, &m.cfg, &w, m.kc.data(), m.vc.data(), out, &arch);
}

void lazy_ctx_destroy(crabml_hip_llama* c) { (void)crabml_hip_llama_destroy(c); }

bool lazy_ctx_orphaned(const crabml_hip_llama* c) {
  // one representative of the model (the first layer's wq; Qwen2: and of its biases, bq) and one of the runner (its first K cache): a
  // handle whose references are all the context's own holds has been released by the host
  auto sole = [&](const crabml_hip_buf* b) {
    if (!b) return false;
    int holds = 0;
    for (const crabml_hip_buf* h : c->held)
      if (h == b) holds++;
    return holds > 0 && b->refcnt.load() <= holds;
  };
  return sole(c->wq.empty() ? nullptr : c->wq[0]) || (c->qwen2 && sole(c->bq[0])) || (c->ext_kv && sole(c->ext_kc0));
}

int lazy_ctx_n_segments(const crabml_hip_llama* c) { return n_segments(c); }

int lazy_ctx_begin(crabml_hip_llama* c, size_t token, size_t pos) {
  if (c->dev->dry) return 0;
  // A token whose shadow is dropped half-way (lazy.hip: the op stream left the template) never reaches the sampler launch that
  // advances the step serial on the device -- and the epochs of the in-launch hand-offs (norm gathers, Q8_K exchanges) are derived
  // from it: the NEXT token's first segments would match the dropped token's granules.  So here the host owns the serial: every
  // begin sets a fresh even value, the sampler's own + 1 lands on the odd one in between.
  c->lazy_serial += 2;
  c->out_seq++;
  k_set_state5<<<1, 1, 0, c->dev->stream>>>(c->state, (int)token, (int)pos, 0, (int)c->lazy_serial, (int)c->out_seq);
  CH_HIP(c->dev, hipGetLastError());
  c->attn_variant = variant_of(c, pos);
  c->kv_len = pos + 1;
  return 0;
}

int lazy_ctx_segment(crabml_hip_llama* c, int seg) {
  if (c->dev->dry) return 0;
  return enqueue_segment(c, seg);
}

// the whole step at once: the context's captured graph (false: this context has none -- the caller enqueues segment by segment)
bool lazy_ctx_has_graph(const crabml_hip_llama* c) { return !c->dev->dry && c->use_graph && c->exec[0] != nullptr; }
int lazy_ctx_step(crabml_hip_llama* c, size_t pos) {
  if (c->dev->dry) return 0;
  return run_step(c, pos);
}

// dst = the logits of the last step (device to device; for a handle the host kept and uses as an operand)
int lazy_ctx_copy_logits(crabml_hip_llama* c, float* dst) {
  if (c->dev->dry) return 0;
  CH_HIP(c->dev, hipMemcpyAsync(dst, c->logits, c->cfg.vocab_size * 4, hipMemcpyDeviceToDevice, c->dev->stream));
  return 0;
}

int lazy_ctx_final_norm(crabml_hip_llama* c, float* dst) {
  crabml_hip_device* dev = c->dev;
  if (dev->dry) return 0;
  const int dim = (int)c->cfg.embedding_dim;
  // the order of the step's own final norm: the reference's scan on a strict-order device, the fast split otherwise
  const int half = dev->strict_order ? 0 : 1;
  launch_norm_f32(dev->stream, c->x, nullptr, (const float*)c->rms_final->ptr, dim, c->cfg.rms_norm_eps, dst, half);
  CH_HIP(dev, hipGetLastError());
  return 0;
}

// the fault word of the in-launch gathers travels with the sync the caller performs anyway: request it before, read it after
int lazy_ctx_fault_request(crabml_hip_llama* c) {
  crabml_hip_device* dev = c->dev;
  if (dev->dry) return 0;
  int* h = c->h_state + crabml_hip_llama::H_STATE_SLOTS * 4;  // pinned, behind the state ring
  CH_HIP(dev, hipMemcpyAsync(h, c->state + 5, sizeof(int), hipMemcpyDeviceToHost, dev->stream));
  return 0;
}
// the logits of the last final segment in pinned host memory: spins on the flag the step's last kernel raises (bounded; then the
// stream is drained the ordinary way).  nullptr: this context has no host copy.
const float* lazy_ctx_wait_logits(crabml_hip_llama* c, int* fault) {
  if (c->dev->dry || c->host_logits == nullptr || c->out_seq == 0) return nullptr;
  volatile unsigned* flag = (volatile unsigned*)(c->host_logits + c->cfg.vocab_size);
  const unsigned want = c->out_seq;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0; __atomic_load_n((const unsigned*)flag, __ATOMIC_ACQUIRE) != want; spins++) {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
    if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
      if (hipStreamSynchronize(c->dev->stream) != hipSuccess) return nullptr;
      if (__atomic_load_n((const unsigned*)flag, __ATOMIC_ACQUIRE) != want) return nullptr;
      break;
    }
  }
  *fault = (int)flag[1];
  return c->host_logits;
}
bool lazy_ctx_has_host_logits(const crabml_hip_llama* c) { return c != nullptr && (c->host_logits != nullptr || c->dev->dry); }
int lazy_ctx_fault_value(const crabml_hip_llama* c) { return c->dev->dry ? 0 : c->h_state[crabml_hip_llama::H_STATE_SLOTS * 4]; }

}  // namespace crabml_hip
