/*
 * crabml_hip_debug.h -- parity hooks, measurement hooks and A/B switches of libcrabml_hip.so.
 *
 * NOT part of the drop-in boundary (include/crabml_hip.h): nothing a crabml maintainer binds lives here.  These entry points
 * and flag bits exist for tests/ (bit-level parity of the production inner loops against the oracle, A/B identity of kernel
 * variants), bench.py (per-kernel event timing, the measured read ceiling) and the labs under tools/.
 */
#ifndef CRABML_HIP_DEBUG_H
#define CRABML_HIP_DEBUG_H

#include "crabml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device flags of the tests (crabml_hip_device_options_t.flags; the public bits are in crabml_hip.h) ---- */
#define CRABML_HIP_FLAG_LAZY_NO_FUSION 4 /* A/B: record the Tensor calls but always run the queue op by op (never match the decode step) */
#define CRABML_HIP_FLAG_DRY 0x40000000  /* test hook, needs CRABML_HIP_TEST_HOOKS=1: a record-only device object with NO HIP device behind
                                           it -- calls are validated, recorded, matched and counted, nothing is computed, export() yields
                                           zeros.  The CPU test suite drives the queue and the matcher through it. */
/* counters of the recorded-op queue (crabml_amd/csrc/lazy.hpp, LazyStats): out[0..7] = ops recorded, ops run one launch at a time,
 * tokens served by the fused step, recorded ops those tokens replaced, fused segments enqueued, shadow tokens aborted, decode
 * contexts built, final-norm rows bound on demand, [8] nanoseconds the host spent blocked in export, [9] exports served from
 * the pinned logits copy requested at commit, [10] parked decode contexts taken back into service (runners taking turns on one
 * device: up to two contexts wait beside the one being served), [11] contexts dropped because the host had released the model or
 * the caches they served (checked after every flush; also dropped: every idle context when a device allocation fails) */
int crabml_hip_debug_lazy_stats(crabml_hip_device_t* dev, uint64_t* out, size_t cap);

/* the host NUMA node the device is attached to (sysfs numa_node of its PCI function), -1 if unknown: bench.py runs its host
 * threads there (a host that drives the device token by token is sensitive to the socket it sits on) */
int crabml_hip_debug_device_numa_node(crabml_hip_device_t* dev, int32_t* node);

/* ---- parity / debug hooks (used by tests; not on the hot path) ------------------------------ */
/* Quantizes the first n f32 elements of x to `qtype` (Q8_0 | Q8_1 | Q8_K) on the device and returns
 * the blocks in the reference's byte layout (buf_q8_0.rs:8-13, buf_q8_1.rs:73-79, buf_q8_k.rs:6-12). */
int crabml_hip_debug_quantize(crabml_hip_device_t* dev, const crabml_hip_buf_t* x, size_t n, uint32_t qtype,
                              void* dst, size_t dst_bytes);
/* Exact integer part of W(row) . X per 32-element group (one int32 each; k/32 values): the
 * bit-exact gate for the nibble unpack + integer dot. */
int crabml_hip_debug_block_dots(crabml_hip_device_t* dev, const crabml_hip_buf_t* w, size_t m, size_t k, size_t row,
                                const crabml_hip_buf_t* x, int32_t* dst);
/* The integers of the PRODUCTION K-quant loops, per super-block (Q4_K / Q6_K weights, Q8_K rhs; north_star: "bit-exactly
 * at the integer unpack level").  The single-row kernels' own inner loops (rows_partial_q4k / rows_partial_q6k in their
 * debug instantiation: the same code k_gemv_q4_k / k_qkv / k_gemv_res_nq / k_gateup_k_lds run) walk row `row` and hand out
 * what their float part consumes: dst[2 sb] = isum = sum_j scale_j * sum(q * q8) and dst[2 sb + 1] = msum = sum_j min_j *
 * bsum_j for Q4_K (buf_q4_k.rs:212-263; variant 0 = quad-exchanged header dwords, 1 = whole-header loads, the form the
 * LDS-staged kernels use); dst[2 sb] = sum_g scale_g * sum((q6 - 32) * q8), dst[2 sb + 1] = 0 for Q6_K
 * (buf_q6_k.rs:183-234).  k / 256 pairs.  *value (optional) = the kernel's own f32 result for the row. */
int crabml_hip_debug_superblock_ints(crabml_hip_device_t* dev, const crabml_hip_buf_t* w, size_t m, size_t k, size_t row,
                                     const crabml_hip_buf_t* x, int32_t variant, int32_t* dst, float* value);
/* The same integers out of the matrix-core GEMM (k_gemm_mfma_q4k / k_gemm_mfma_q6k themselves, run with their dump
 * pointer set): x holds b >= 16 rows of k; dst[((bi * m + row) * (k / 256) + sb) * 2 + {0, 1}] = (isum, msum) for Q4_K and
 * (sum_g scale_g * sum(q6 * q8), sum_g scale_g * bsum_g) for Q6_K -- the -32 offset is applied as isum - 32 * that.
 * out (optional, b * m floats) receives the GEMM's f32 result. */
int crabml_hip_debug_gemm_ints(crabml_hip_device_t* dev, const crabml_hip_buf_t* w, size_t m, size_t k,
                               const crabml_hip_buf_t* x, size_t b, int32_t* dst, float* out);
/* The fast prompt pass's weight GEMM (k_gemm_f16w, gemm_f16w.hip) by itself.  w: nw = 1..3 weight buffers of one format (Q4_0,
 * Q8_0, Q4_1, Q4_K, Q6_K, Q2_K, Q3_K, Q5_K), m[j] rows of k; x: b >= 16 f32 rows of k.  The rows are quantized to the format's row type (Q8_0 / Q8_1 /
 * Q8_K) and B' (the pre-scaled f16 rows the GEMM reads) is written by the quantizer itself (rows_path 0) or made from the finished
 * planes by k_rows_to_f16 (1) -- into an allocation of the product's size (gemm_f16w_xh_bytes) whose every 16-bit word holds `junk`
 * before.  force[4] (nullable) = F (1 | 2), T (2 | 4 | 8), ksplit (1 | 2 | 4 | 8), gate | up (0 off, 1 h = silu(g) * u as f32, 2 h
 * as row planes + ffn_down's B'); 0 (gate | up: -1) = the launcher's own choice.  out[j]: b * m[j] f32 (gate | up: out[0] = h,
 * out[1] untouched).  xh (nullable): the b * k halfs of B' the kernel read, in its k-slot order.  used[8] (nullable): F, T, ksplit,
 * gate | up as launched, the B' overflow flag (1: some value written to B' was +-inf), then off_d, off_aux, total of h's row planes.
 * hq (nullable, gate | up 2): b * total bytes of h's row planes; hxh (nullable): b * m[0] halfs of ffn_down's B'.  A shape, forced
 * launch form or weight scales the GEMM does not take: CRABML_HIP_NOT_IMPLEMENTED.  Host pointers; blocks. */
int crabml_hip_debug_gemm_f16w(crabml_hip_device_t* dev, const crabml_hip_buf_t* const* w, const size_t* m, size_t nw, size_t k,
                               const crabml_hip_buf_t* x, size_t b, int32_t rows_path, uint16_t junk, const int32_t* force,
                               float* const* out, uint16_t* xh, int32_t* used, void* hq, uint16_t* hxh);
/* Sustained HBM read rate of this device as a plain streaming kernel reaches it (16-byte non-temporal loads over `bytes`
 * bytes, best of `reps` launches, HIP events on the device stream): the practical ceiling bench.py quotes next to the
 * 8 TB/s datasheet peak. */
int crabml_hip_debug_read_ceiling(crabml_hip_device_t* dev, size_t bytes, int32_t reps, double* gbytes_per_s);

/* The fast step's long-context attention (k_attn_flash + k_attn_flash_merge, fused_attention.hpp) by itself: one query row per
 * head against `seq` cached positions.  q: n_heads * head_dim f32 (already scaled; rounded to f16 by the kernel as
 * batch_matmul.rs:39 does); k, v: [n_kv][seq_cap][head_dim] f16 bits; slices: the grid's position slices per kv head (1 .. 32; a
 * step uses as many as the context repays); out: n_heads * head_dim f32 = softmax(q k^T) v in f32 arithmetic, from the shipped
 * two-launch form.  out2 (nullable): the same from the single-launch form (the last-arriving workgroup of a kv head merges;
 * launched twice on the same ticket words, which the last arriver re-arms).  n_heads / n_kv from 1 to 8 at head_dim 64 / 128,
 * 1 / 2 / 4 / 8 at head_dim 256; anything else: BAD_INPUT.  seq_cap >= seq: the rows of a kv head in k and v, [n_kv][seq_cap][head_dim],
 * handed to both kernels as the cache row stride -- positions 0 .. seq - 1 are live, whatever lies beyond must not matter.  Host
 * pointers; blocks. */
int crabml_hip_debug_flash_attention(crabml_hip_device_t* dev, const float* q, const uint16_t* k, const uint16_t* v, size_t n_heads,
                                     size_t n_kv, size_t head_dim, size_t seq, size_t seq_cap, size_t slices, float* out, float* out2);

/* The fast prompt pass's causal attention (k_attn_flash_rows: flash attention on the f16 matrix cores) by itself.  q: rows *
 * n_heads * head_dim f32 (row r is the prompt row at position pos0 + r); k, v: [n_kv][seq_cap][head_dim] f16 bits (the cache
 * after the pass's appends: positions 0 .. pos0 + rows - 1 are live, whatever lies beyond must not matter); out: rows * n_heads *
 * head_dim f32, row r = softmax(q_r k^T over positions 0 .. pos0 + r) v.  head_dim 64 / 128.  Host pointers; blocks. */
int crabml_hip_debug_flash_attention_rows(crabml_hip_device_t* dev, const float* q, const uint16_t* k, const uint16_t* v, size_t n_heads,
                                          size_t n_kv, size_t head_dim, size_t pos0, size_t rows, size_t seq_cap, float* out);

/* The decode step's sampler (crabml_hip_llama_decode_sample: k_sample_max / k_sample_keys / k_sample_pick, or the arg-max
 * kernels at temperature 0) on n arbitrary f32 logits (host pointer) with one coin, on this device's tier (strict order:
 * the reference's token bit for bit).  Same argument checks and errors as decode_sample.  Blocks. */
int crabml_hip_debug_sample(crabml_hip_device_t* dev, const float* logits, size_t n, float temperature, float topp, float coin,
                            uint32_t* token);

/* ---- A/B switches and test hooks of the fused decode step (crabml_hip_llama_config_t.flags; the public bits are in
 * crabml_hip.h).  Every variant pair is bit-identical unless its comment says otherwise. */
#define CRABML_HIP_LLAMA_NO_NORM_EPILOGUE 4 /* A/B: keep RMSNorm + quantize as its own launch (fast mode runs it in
                                              the wo / ffn_down epilogue; bit-identical either way) */
#define CRABML_HIP_LLAMA_NO_KQUANT_FUSION 256 /* A/B: Q4_K / Q4_1 layers through the per-op segment path */
#define CRABML_HIP_LLAMA_Q4_1_SEGMENTS 512 /* A/B: Q4_1 layers as 11 launches (separate norm / quantize launches) */
#define CRABML_HIP_LLAMA_NO_TILE_ATTENTION 2048 /* A/B: prefill attention as one workgroup per (head, row) */
#define CRABML_HIP_LLAMA_NO_RHS_PROLOGUE 1024 /* A/B: Q4_K layers quantize the rhs of wo / ffn_down in its own launch */
#define CRABML_HIP_LLAMA_TP_DRY_RUN 128 /* measurement hook: a lone tp rank (tp_comm = NULL) steps with its all-reduces
                                          skipped -- per-rank kernel time of a tp group; the logits are meaningless */
#define CRABML_HIP_LLAMA_NO_LONG_ATTENTION 64 /* A/B: one attention workgroup per head at every context length */
#define CRABML_HIP_LLAMA_NO_Q8K_PRODUCERS 32768 /* A/B: Q4_K layers quantize the rhs of wo / ffn_down in those kernels' prologues instead
                                                  of receiving finished Q8_K planes from attention / gate-up (bit-identical) */
#define CRABML_HIP_LLAMA_Q8K_ATTN_PRODUCER 65536 /* A/B, opt-in: the staged attention kernel also assembles wo's Q8_K planes (pairs of heads
                                                   exchange their outputs); measured slower than wo's own 4096-element prologue */
#define CRABML_HIP_LLAMA_NO_PV_PRODUCER_WAVES 131072 /* A/B: long-context decode runs k_attn_pv (the chain wave multiplies and adds)
                                                       instead of k_attn_pv_split (producer waves multiply); bit-identical */
#define CRABML_HIP_LLAMA_NO_PREFILL_ROW_FUSION 262144 /* A/B: the prompt pass keeps residual-add / RMSNorm / quantize and SiLU * mul / quantize as
                                                        separate launches (bit-identical) */
#define CRABML_HIP_LLAMA_NO_PV_ROW_TILES 16384 /* A/B: long-prompt prefill runs the PV pass one prompt row per workgroup */
#define CRABML_HIP_LLAMA_NO_STAGED_ATTENTION 8192 /* A/B: short-context attention without the LDS staging of K / V (k_attn) */
#define CRABML_HIP_LLAMA_FLASH_TICKET 2097152 /* A/B: k_attn_flash merges its partials in the last-arriving workgroup of a kv head
                                                (ticket word, write-through hand-off) instead of a second launch */
#define CRABML_HIP_LLAMA_NO_H_CONSUMER_QUANT 4096 /* A/B, tensor-parallel ranks: gate/up quantizes h itself (hidden / tp / 32 workgroups of 32 rows, k_gateup_q)
                                                   instead of leaving h as f32 from one workgroup per CU for ffn_down's prologue (bit-identical) */
#define CRABML_HIP_LLAMA_PREFILL_INT8_GEMM 524288 /* A/B: the fast prompt pass keeps the bit-exact int8 matrix-core GEMM (with the fused last
                                                     product) at every pass size, instead of the weight-stationary f16 GEMM that Q4_0 / Q8_0 /
                                                     Q4_1 / Q4_K / Q6_K / Q2_K / Q3_K weights take from 32 rows (gemm_f16w.hip; a stated deviation of the
                                                     fast tier) -- and Q5_K weights in a context created with
                                                     CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM, which this flag overrides */
#define CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM 536870912 /* opt-in kernel variant (NOT bit-identical): fast mode, one device, prompt passes of 32 rows
                                                      or more run Q5_K matrices on the weight-stationary f16 matrix-core GEMM the other
                                                      K-quants take by default (gemm_f16w.hip; A' = f16(q f16(d sc) - f16(dmin m)), a stated
                                                      deviation of the fast tier like Q4_K's) instead of the row-by-row GEMV.
                                                      Off, a Q5_K matrix runs exactly as it always has (the launch pins of the K-quant passes
                                                      state that); on a model without Q5_K tensors the flag changes nothing.  Strict-order
                                                      devices, tensor parallelism, matmul_vec, shorter passes and decode ignore it;
                                                      CRABML_HIP_LLAMA_PREFILL_INT8_GEMM overrides it.  Declared here because the public
                                                      header holds its eight flag bits already; tools/generate.py --q5k-gemm sets it */
#define CRABML_HIP_LLAMA_PREFILL_TAP_Q2K_Q3K 268435456 /* test hook: crabml_hip_llama_debug_prefill_tap also serves contexts whose layer
                                                         matrices or classifier are Q2_K / Q3_K (the checker restates their kernels:
                                                         tests/q23k_f16w_ref.py).  Off, the tap refuses such a context with
                                                         NOT_IMPLEMENTED, as it always has.  Changes nothing the pass computes */
#define CRABML_HIP_LLAMA_PREFILL_SEPARATE_F16_ROWS 33554432 /* A/B, fast prompt pass: the rows' f16 planes for the weight GEMM are made by their
                                                              own launch (k_rows_to_f16) instead of by the kernels that quantize the rows,
                                                              and the k pieces of a split wo / ffn_down GEMM are added by their own launch
                                                              (k_addn_f32) instead of by the norm kernel that consumes them (bit-identical) */
#define CRABML_HIP_LLAMA_PREFILL_NO_GU_EPILOGUE 67108864 /* A/B, fast prompt pass: gate | up leave g and u and SiLU * mul (+ quantize) stays its own
                                                           launch, instead of being the f16 GEMM's epilogue (bit-identical) */
#define CRABML_HIP_LLAMA_NO_K_NORM_IN 16777216 /* A/B, fast Q4_K step: wo gathers the row's sums and quantizes its output to Q8_K itself (two
                                                  in-launch hops) instead of leaving x for gate | up to normalize and quantize (bit-identical) */
#define CRABML_HIP_LLAMA_SPLIT_CHUNKS_ALWAYS 16 /* test / tuning hooks for the norm epilogue: two workgroups per */
#define CRABML_HIP_LLAMA_SPLIT_CHUNKS_NEVER 32  /* 32-row chunk always / never (default: only for long rows)   */
#define CRABML_HIP_LLAMA_NQ_TWO_UNIT_ROUNDS 134217728 /* A/B, fast Q4_0 / Q8_0 / Q4_1 step: ffn_down / wo keep two-unit request rounds (every wave reads
                                                         its rhs units from global memory: request two 64-unit steps of a row, wait, consume,
                                                         repeat) where the launch would copy the rhs planes into LDS once per workgroup and
                                                         request the row's weights ahead (rows_partial_deep; bit-identical) */

/* parity hook: copies the layer's K or V cache (raw f16/f32 bytes, [n_kv_heads][seq_len][head_dim]) */
int crabml_hip_llama_debug_kv(crabml_hip_llama_t* ctx, size_t layer, int32_t which_v, void* dst, size_t nbytes);

/* test hook: fills what no launch may consume, on the context's stream (stream-ordered with the steps and passes around it; does
 * not block).  The invariant it serves: no launch's result depends on cache rows past the live positions or on
 * scratch bytes it did not write in the same step or pass.  fill16 goes to f16 data and, repeated, to the quantized activation
 * planes (their scale fields then read as the pattern); fill32 to f32 data.  A buffer is filled as the whole allocation behind it.
 *   what & 1, the cache tail: rows kv_len .. seq_len - 1 of every layer and kv head, K and V (f16 cache: fill16, f32 cache: fill32).
 *   what & 2, the step's data scratch -- every buffer a step writes before it reads it:
 *     fill32: x (k_embed writes it first), partial (unused on one device), qbuf, attn, h, tmp, xn, logits, rsums, scores_g,
 *             flash_part (the merge reads the active slices' partials only), am_val (all ARGMAX_BLOCKS written by k_argmax_partial),
 *             out_tokens (read by the host only, the entries of the call's own steps);
 *     fill16: act_dim, act_attn, act_hid (every plane of a set is written by its producer), p16.
 *   what & 4, the prompt pass's row buffers, if allocated (otherwise nothing):
 *     fill32: pf_x, pf_xn, pf_q, pf_k, pf_v, pf_qr, pf_attn, pf_tmp, pf_g, pf_u, pf_split, pf_scores;
 *     fill16: pf_act_dim, pf_act_hid, pf_xh, pf_xh2 (B': rows past the pass feed output rows nobody reads), pf_p16.
 * Never written, in any mode:
 *   state, slots, a8gran, h8gran, flash_tick, pf_ovf, the sampler's histogram, the inboxes of a P2P group: words that kernels poll or
 *     count on from one launch to the next (epochs, tickets, the fault word, token / pos / step);
 *   am_best (what a vocabulary-split group combines after the step), am_idx and pf_tokens (indices: the next launch addresses the
 *     embedding table with them -- a stale one must not become an address), the rope, exp and gelu tables, the weights;
 *   the sampler's sm_bmax / sm_keys / sm_par / sm_coins: allocated by the first decode_sample, not at create; par and coins are
 *     uploaded by every call (reuse of a sampling context is held by tests/test_hip_reuse_equals_fresh.py without the hook);
 *   the tap scratch areas (written and read back inside one hook call).
 * No buffer of a context carries DATA from one step to the next outside the cache and the words above.
 * Tensor-parallel ranks and a context on the runner's own KV cache (the recorded-op queue owns those): CRABML_HIP_NOT_IMPLEMENTED. */
int crabml_hip_llama_debug_poison(crabml_hip_llama_t* ctx, uint32_t what, uint16_t fill16, uint32_t fill32);

/* parity hook: ONE decode step for (token, pos) -- the same checks and the same effect on the context as
 * crabml_hip_llama_forward -- enqueued EAGERLY (never replayed from the step's hipGraph, never while capturing), with the buffers
 * of layer `layer` copied out as each launch of that layer left them: stream-ordered device-to-device copies into a scratch area
 * (allocated on the first tap of a context) placed between the launches, brought to the host after the step.  The step runs to
 * its end as always; logits (vocab_size floats, nullable) come back as from forward.  Serves the five-launch layers of
 * enqueue_segment_t (Q4_0 / Q8_0 / Q4_1) and the K-quant layers of enqueue_segment_k (Q4_K, the Q4_K_M mix, Q5_K and Q5_K_M, an
 * all-Q6_K body, the Q3_K family (Q3_K_S / _M / _L) and the Q2_K family (plain Q2_K, the Q2_K / Q2_K_S recipes), Q4_1 in front of a
 * classifier of another format) on one device, fast tier; tensor-parallel ranks, the per-op path, the strict-order device and a
 * context the recorded-op queue drives on the runner's own KV cache return CRABML_HIP_NOT_IMPLEMENTED.
 * dst / dir: field f occupies dir[f].bytes bytes at dst + dir[f].offset (bytes = 0: the context has no such buffer, e.g. rsums
 * outside the hop-free form).  f32 fields are raw floats.  Quantized rows come back in the reference's block byte layout, as
 * crabml_hip_debug_quantize returns them: Q8_0 block i = d plane [i] (f16) | q plane [32 i .. 32 i + 31]; Q8_1 = d plane [i] |
 * third plane [i] (s, f16) | q plane; Q8_K = d plane [i] (f32) | q plane [256 i ..] | bsums plane [16 i ..] -- the Q8_0 layout's
 * third plane (the blocks' integer sums, a kernel-side convenience) is not part of a block and is left out.  The fourth plane of a
 * Q8_K set (the class-major copy of the quants that the Q4_K kernels read, common.hpp) leaves as a raw field of its own (the _QP
 * fields: cols bytes).  On the K-quant path a plane field is copied only where a launch wrote the set to global memory (bytes = 0
 * where the consuming kernel quantizes in its prologue or in LDS).
 * dst == NULL: nothing runs, *need receives the bytes dst must hold. */
enum {
  CRABML_HIP_TAP_QKV_IN_X = 0,      /* what the q|k|v launch of the layer reads: x (f32, dim), */
  CRABML_HIP_TAP_QKV_IN_ACT = 1,    /*   the act_dim planes (layer row type), */
  CRABML_HIP_TAP_QKV_IN_RSUMS = 2,  /*   rsums (f32, dim / 32 chunk sums of squares; stale bytes in front of layer 0) */
  CRABML_HIP_TAP_QBUF = 3,          /* after q|k|v: qbuf (f32, dim); the K / V rows at pos: crabml_hip_llama_debug_kv */
  CRABML_HIP_TAP_ATTN = 4,          /* after attention (and the stand-alone quantizer, head_dim % 32 != 0): attn (f32, dim), */
  CRABML_HIP_TAP_ACT_ATTN = 5,      /*   the act_attn planes */
  CRABML_HIP_TAP_WO_X = 6,          /* what the gate|up launch reads, i.e. after wo (and the norm launch, NO_NORM_EPILOGUE): x, */
  CRABML_HIP_TAP_WO_ACT = 7,        /*   the act_dim planes, */
  CRABML_HIP_TAP_WO_RSUMS = 8,      /*   rsums */
  CRABML_HIP_TAP_ACT_HID = 9,       /* after gate|up: the act_hid planes (hidden) */
  CRABML_HIP_TAP_DOWN_X = 10,       /* after ffn_down: x, */
  CRABML_HIP_TAP_DOWN_ACT = 11,     /*   the act_dim planes (NO_NORM_EPILOGUE: after the norm launch of the next segment; 0 bytes when
                                         that launch writes another row type, i.e. in front of a classifier of its own format), */
  CRABML_HIP_TAP_DOWN_RSUMS = 12,   /*   rsums */
  CRABML_HIP_TAP_CLS_ACT = 13,      /* last segment, any `layer`: what the classifier reads (the classifier's row type; f32 for an F32 / F16 classifier) */
  CRABML_HIP_TAP_PLAN = 14,         /* CRABML_HIP_TAP_PLAN_WORDS int32 words: the launch plan of the tapped step as the host took it (below) */
  /* the K-quant layers (enqueue_segment_k) */
  CRABML_HIP_TAP_GATEUP_H = 15,     /* after gate|up: h (f32, hidden), which every K form of the launch writes */
  CRABML_HIP_TAP_QKV_IN_XN = 16,    /* the f32 row of the stand-alone norm launch in front of q|k|v (layer 0; every layer without the norm epilogue), */
  CRABML_HIP_TAP_WO_XN = 17,        /*   ... in front of gate|up (without the norm epilogue), */
  CRABML_HIP_TAP_CLS_XN = 18,       /*   ... in front of the classifier (without the norm epilogue) */
  CRABML_HIP_TAP_QKV_IN_QP = 19,    /* the class-major plane of QKV_IN_ACT, */
  CRABML_HIP_TAP_ACT_ATTN_QP = 20,  /*   of ACT_ATTN, */
  CRABML_HIP_TAP_WO_QP = 21,        /*   of WO_ACT, */
  CRABML_HIP_TAP_ACT_HID_QP = 22,   /*   of ACT_HID, */
  CRABML_HIP_TAP_DOWN_QP = 23,      /*   of DOWN_ACT, */
  CRABML_HIP_TAP_CLS_QP = 24,       /*   of CLS_ACT; each 0 bytes where the set is not Q8_K or was not written */
  CRABML_HIP_TAP_FIELDS = 25
};
/* On the K-quant path WO_RSUMS is what the NORMIN gate|up launch reads: wo's chunk sums of squares, PLAN_SPLIT_WO per 32-row chunk
 * (f32, dim / 32 * split; 0 bytes unless PLAN_WO_X_ONLY), and WO_ACT is 0 bytes there (the planes exist in LDS only). */
/* the words of CRABML_HIP_TAP_PLAN, written by the enqueue code where it decides (0 where the tapped layer never got there) */
enum {
  CRABML_HIP_PLAN_N_CU = 0,         /* compute units of the device (what dim / 32 and split_of() are compared with) */
  CRABML_HIP_PLAN_DEFER_NORM = 1,   /* 1: the context runs the hop-free norm */
  CRABML_HIP_PLAN_NORM_EPILOGUE = 2,/* 1: RMSNorm + quantize run in the wo / ffn_down epilogue */
  CRABML_HIP_PLAN_ATTN_VARIANT = 3, /* 0 one workgroup per head, 1 the long-context kernels, 2 the same with the merge in the launch; + 16 when those are k_attn_flash */
  CRABML_HIP_PLAN_SPLIT_WO = 4,     /* workgroups per 32-row chunk of the layer's wo launch (split_of(k)), 0 without the norm epilogue */
  CRABML_HIP_PLAN_SPLIT_DOWN = 5,   /* ... of its ffn_down launch */
  CRABML_HIP_PLAN_QKV_LOADER = 6,   /* the row loader k_qkv takes: 1 rows_dot, 2 rows_partial_2step, 3 rows_partial_rms, 4 rows_partial_rms_128 */
  CRABML_HIP_PLAN_NORM_NIT = 7,     /* template argument of the layer's own norm launch in front of q|k|v (4, or 12 for rows past 4096), 0 = none */
  CRABML_HIP_PLAN_PATH = 8,         /* 1 the five launches (enqueue_segment_t), 2 the K-quant launches (enqueue_segment_k); the words below: path 2 */
  CRABML_HIP_PLAN_NORM_EPI_K = 9,   /* 1: wo / ffn_down of the Q4_K layers normalize and quantize to Q8_K in their epilogue */
  CRABML_HIP_PLAN_Q8K_PRODUCERS = 10, /* 1: the context lets attention / gate|up emit the Q8_K planes of wo's / ffn_down's rhs */
  CRABML_HIP_PLAN_K_NORM_IN = 11,   /* 1: the context lets gate|up normalize and quantize wo's f32 row itself */
  CRABML_HIP_PLAN_QIN = 12,         /* 1: wo / ffn_down take their rhs in the prologue (f32 or finished planes), no quantizer launch */
  CRABML_HIP_PLAN_QMODE_WO = 13,    /* the layer's wo launch: 0 rhs planes from global memory, 1 the f32 rhs quantized in the prologue, 2 finished planes copied */
  CRABML_HIP_PLAN_QMODE_DOWN = 14,  /* ... its ffn_down launch */
  CRABML_HIP_PLAN_WO_X_ONLY = 15,   /* 1: wo left x and its chunk sums only, gate|up ran its NORMIN form */
  CRABML_HIP_PLAN_AQ8 = 16,         /* 1: the attention launch produced wo's Q8_K planes */
  CRABML_HIP_PLAN_V_Q6K = 17,       /* 1: the layer's attn_v is Q6_K (a *_K_M mix), */
  CRABML_HIP_PLAN_DOWN_Q6K = 18,    /*   its ffn_down */
  CRABML_HIP_TAP_PLAN_WORDS = 19
};
typedef struct crabml_hip_tap_entry {
  uint64_t offset, bytes;
  uint32_t qtype;     /* CRABML_HIP_F32 or the row type of the blocks */
  uint32_t reserved;
} crabml_hip_tap_entry_t;
int crabml_hip_llama_debug_tap(crabml_hip_llama_t* ctx, size_t token, size_t pos, size_t layer, float* logits, void* dst,
                               size_t dst_bytes, crabml_hip_tap_entry_t* dir, size_t* need);

/* parity hook: ONE chunk pass of the batched prompt path (prefill_chunk_pass) for `n` tokens appended at the current cache length
 * (pos0 = crabml_hip_llama_kv_len) -- the same checks and the same effect on the context as crabml_hip_llama_prefill, including the
 * recomputation of a chunk whose f16 rows overflowed --, with the row buffers of layer `layer` (all n rows of each) copied out as each
 * launch of that layer left them: stream-ordered device-to-device copies into a scratch area (allocated on the first prefill tap of a
 * context, grown when a longer pass is tapped) placed between the launches, brought to the host after the pass.  n larger than the
 * context's chunk capacity (prefill_chunk, else 1024, never more than seq_len): CRABML_HIP_BAD_INPUT -- multi-chunk situations are made
 * by calling prefill / forward first.  Serves Q4_0 / Q8_0 / Q4_1 layers (Q8_0 / Q8_1 rows) and Q8_K-row passes
 * whose layer matrices are Q4_K, Q5_K or Q6_K (the Q4_K_M / Q5_K_M mixes and a Q6_K classifier included) on one fast device, Llama and
 * Qwen2, f16 and f32 cache; every other format (Q8_K weights, Q2_K, Q3_K, Q5_0, Q5_1, F32), tensor-parallel ranks, the strict-order
 * device and a context on the runner's own KV cache return CRABML_HIP_NOT_IMPLEMENTED.  dst / dir / need as for crabml_hip_llama_debug_tap; a field the pass did not produce has bytes = 0.
 * f32 fields are [n][cols] floats.  Quantized rows come back as n rows of blocks in the reference's byte layout (as debug_tap).  The
 * XH fields are the rows' pre-scaled f16 planes B' ([n][cols] halfs, in the GEMM's k-slot order: within a 32-element block the order
 * is the kernel's own business) as the GEMM that reads them next finds them; 0 bytes in an int8 / GEMV pass.  PARTS fields are
 * `parts` consecutive [n][dim] f32 pieces of a GEMM cut along k whose sum was left to the norm launch (piece 0 is the TMP field).
 * The K / V rows come through crabml_hip_llama_debug_kv. */
enum {
  CRABML_HIP_PFTAP_IN_X = 0,       /* what the layer's first norm launch reads: pf_x (f32, dim), */
  CRABML_HIP_PFTAP_IN_TMP = 1,     /*   the previous layer's ffn_down output not yet added (f32, dim; 0 bytes when none is pending), */
  CRABML_HIP_PFTAP_IN_PARTS = 2,   /*   and its k pieces 1.. (PLAN_IN_PARTS of them) */
  CRABML_HIP_PFTAP_N1_X = 3,       /* what it leaves: pf_x, */
  CRABML_HIP_PFTAP_N1_ACT = 4,     /*   the act_dim planes (layer row type), */
  CRABML_HIP_PFTAP_N1_XH = 5,      /*   B' as the q|k|v GEMM reads it */
  CRABML_HIP_PFTAP_Q = 6,          /* after the q|k|v GEMM(s): pf_q (dim), */
  CRABML_HIP_PFTAP_K = 7,          /*   pf_k (kv_dim), */
  CRABML_HIP_PFTAP_V = 8,          /*   pf_v (kv_dim) */
  CRABML_HIP_PFTAP_QR = 9,         /* after k_qkv_epi_rows: pf_qr (roped, scaled q; dim) */
  CRABML_HIP_PFTAP_ATTN = 10,      /* after attention: pf_attn (dim), */
  CRABML_HIP_PFTAP_ATTN_ACT = 11,  /*   then its planes */
  CRABML_HIP_PFTAP_ATTN_XH = 12,   /*   and B' as wo's GEMM reads it */
  CRABML_HIP_PFTAP_WO_TMP = 13,    /* after wo: pf_tmp (dim; piece 0 when PLAN_WO_PARTS > 0), */
  CRABML_HIP_PFTAP_WO_PARTS = 14,  /*   the pieces left to the norm launch */
  CRABML_HIP_PFTAP_N2_X = 15,      /* after the residual add + FFN norm: pf_x, */
  CRABML_HIP_PFTAP_N2_ACT = 16,    /*   the act_dim planes, */
  CRABML_HIP_PFTAP_N2_XH = 17,     /*   B' as the gate|up GEMM reads it */
  CRABML_HIP_PFTAP_G = 18,         /* after gate|up: pf_g (hidden): g, or h = silu(g) * u when PLAN_H_DONE == 1; 0 bytes when PLAN_H_DONE == 2 */
  CRABML_HIP_PFTAP_U = 19,         /*   pf_u (hidden); 0 bytes when PLAN_H_DONE != 0 */
  CRABML_HIP_PFTAP_HID_ACT = 20,   /* the act_hid planes (hidden) */
  CRABML_HIP_PFTAP_HID_XH = 21,    /*   and B' as ffn_down's GEMM reads it */
  CRABML_HIP_PFTAP_DOWN_TMP = 22,  /* after ffn_down: pf_tmp (piece 0 when PLAN_DOWN_PARTS > 0), */
  CRABML_HIP_PFTAP_DOWN_PARTS = 23,/*   the pieces left to the next layer's norm launch */
  CRABML_HIP_PFTAP_DOWN_X = 24,    /*   pf_x where the residual was added by k_res_epi right behind it (the last layer; every layer without row fusion) */
  CRABML_HIP_PFTAP_LAST_X = 25,    /* any `layer`: the row the final norm reads (f32, dim), */
  CRABML_HIP_PFTAP_CLS_ACT = 26,   /*   what the classifier reads (one row of the classifier's row type; f32 for an F32 / F16 classifier) */
  CRABML_HIP_PFTAP_PLAN = 27,      /* CRABML_HIP_PFTAP_PLAN_WORDS int32 words (below) */
  /* the fields below: 0 bytes where the arm that makes them did not run */
  CRABML_HIP_PFTAP_N1_XN = 28,     /* pf_xn after the layer's first norm (f32, dim): written by k_norm_f32_rows (separate launches) and by
                                      k_norm_quant_rows_k; 0 bytes behind the Q8_0 / Q8_1 row kernels, which never store it */
  CRABML_HIP_PFTAP_N2_XN = 29,     /*   ... after the FFN norm */
  CRABML_HIP_PFTAP_HID_H = 30,     /* pf_g after k_gateup_epi (f32, hidden): h over g, in the arm where g and u were stored (PLAN_H_DONE == 0,
                                      no SiLU * mul + quantize row kernel) */
  CRABML_HIP_PFTAP_N1_XH_V = 31,   /* B' as v's GEMM reads it, where that GEMM re-made pf_xh (another k-slot order than q's: a Q6_K attn_v
                                      behind a Q4_K attn_q; or q took no f16 GEMM at all: a Q5_K attn_q) */
  CRABML_HIP_PFTAP_CLS_XN = 32,    /* the final norm's f32 row (dim) */
  CRABML_HIP_PFTAP_N1_QP = 33,     /* Q8_K rows only: the class-major plane of the N1_ACT planes, [n][dim] bytes (byte 4 (e % 8) + e / 8 of a
                                      32-group holds element e), */
  CRABML_HIP_PFTAP_ATTN_QP = 34,   /*   of ATTN_ACT, */
  CRABML_HIP_PFTAP_N2_QP = 35,     /*   of N2_ACT, */
  CRABML_HIP_PFTAP_HID_QP = 36,    /*   of HID_ACT ([n][hidden]), */
  CRABML_HIP_PFTAP_CLS_QP = 37,    /*   of CLS_ACT (a Q8_K classifier row; [dim]) */
  CRABML_HIP_PFTAP_FIELDS = 38
};
/* the words of CRABML_HIP_PFTAP_PLAN, written by prefill_chunk_pass where it decides (0 where the tapped layer never got there) */
enum {
  CRABML_HIP_PFPLAN_N_CU = 0,        /* compute units of the device */
  CRABML_HIP_PFPLAN_ROWS = 1,        /* rows of the pass */
  CRABML_HIP_PFPLAN_POS0 = 2,        /* position of row 0 */
  CRABML_HIP_PFPLAN_F16W = 3,        /* 1: the weight-stationary f16 GEMM; 0: the int8 matrix-core GEMM / the GEMV */
  CRABML_HIP_PFPLAN_RECOMPUTED = 4,  /* 1: the tapped pass is the int8 recomputation after an f16 pass raised the overflow flag */
  CRABML_HIP_PFPLAN_NORM_KERNEL = 5, /* the layer's FIRST norm launch (attention norm), noted in the arm that launches it: 0 separate launches
                                        (k_res_epi, k_norm_f32_rows, the quantizer), 1 k_norm_quant_rows, 2 k_norm_quant_rows_h, 3 k_norm_quant_rows_w
                                        4 k_norm_quant_rows_k (Q8_K rows, from 192 rows of a pass whose dim is whole super-blocks: residual add, the k
                                        pieces, RMSNorm and the wave-per-super-block Q8_K quantizer as one launch).  The FFN norm's kernel is not
                                        recorded: it goes through the same arms with wo's pending output and pieces */
  CRABML_HIP_PFPLAN_IN_PARTS = 6,    /* k pieces the layer's first norm launch added to the pending ffn_down output */
  CRABML_HIP_PFPLAN_QKV_ONE = 7,     /* 1: q | k | v as one GEMM launch */
  CRABML_HIP_PFPLAN_GU_ONE = 8,      /* 1: gate | up as one GEMM launch */
  CRABML_HIP_PFPLAN_H_DONE = 9,      /* 0 the launch left g and u, 1 h as f32, 2 h as row planes (+ ffn_down's B') */
  CRABML_HIP_PFPLAN_WO_PARTS = 10,   /* pieces of wo's GEMM left to the norm launch (0: none cut, or added by the GEMM's own reduce launch) */
  CRABML_HIP_PFPLAN_DOWN_PARTS = 11, /* ... of ffn_down's */
  CRABML_HIP_PFPLAN_QKV_F = 12,      /* F (row fragments per wave), T (column tiles per wave), ksplit of the f16 GEMM as launched: q|k|v */
  CRABML_HIP_PFPLAN_QKV_T = 13,      /*   (three separate launches: q's), */
  CRABML_HIP_PFPLAN_QKV_KSPLIT = 14,
  CRABML_HIP_PFPLAN_WO_F = 15,       /*   wo, */
  CRABML_HIP_PFPLAN_WO_T = 16,
  CRABML_HIP_PFPLAN_WO_KSPLIT = 17,
  CRABML_HIP_PFPLAN_GU_F = 18,       /*   gate|up (two separate launches: gate's), */
  CRABML_HIP_PFPLAN_GU_T = 19,
  CRABML_HIP_PFPLAN_GU_KSPLIT = 20,
  CRABML_HIP_PFPLAN_DOWN_F = 21,     /*   ffn_down; all 0 in an int8 / GEMV pass */
  CRABML_HIP_PFPLAN_DOWN_T = 22,
  CRABML_HIP_PFPLAN_DOWN_KSPLIT = 23,
  CRABML_HIP_PFPLAN_ATTN_KERNEL = 24,/* 1 k_attn_flash_rows, 2 the exact tile kernel, 3 the exact long-row kernels, 4 k_attn per (head, row) */
  CRABML_HIP_PFPLAN_KERNEL_Q = 25,   /* the kernel each matrix of the layer took: 1 k_gemm_f16w, 2 the int8 matrix-core GEMM (k_gemm_mfma*), 3 the */
  CRABML_HIP_PFPLAN_KERNEL_K = 26,   /*   wave-per-row GEMV, row by row.  One word per matrix: a launch_gemm_f16w that declines falls through to */
  CRABML_HIP_PFPLAN_KERNEL_V = 27,   /*   launch_gemv, which takes the int8 GEMM from 16 rows where the format has one.  PLAN_F16W says what the */
  CRABML_HIP_PFPLAN_KERNEL_WO = 28,  /*   pass allows, these words what ran (a Q5_K matrix: always 3; the Q6_K matrices of the same layer: 1) */
  CRABML_HIP_PFPLAN_KERNEL_GATE = 29,
  CRABML_HIP_PFPLAN_KERNEL_UP = 30,
  CRABML_HIP_PFPLAN_KERNEL_DOWN = 31,
  CRABML_HIP_PFTAP_PLAN_WORDS = 32
};
int crabml_hip_llama_debug_prefill_tap(crabml_hip_llama_t* ctx, const uint32_t* tokens, size_t n, size_t layer, float* logits, void* dst,
                                       size_t dst_bytes, crabml_hip_tap_entry_t* dir, size_t* need);

/* test hook: what a decode context of this configuration would run.  Creates the context exactly as crabml_hip_llama_create_arch
 * does (arch nullable = Llama), copies its step plan -- the one value that says which segment enqueuer, which segment forms and which
 * attention forms the context takes -- into `words` (CRABML_HIP_STEPPLAN_WORDS of them; n_words smaller: CRABML_HIP_BAD_INPUT),
 * destroys the context and returns create's own return code (on an error the words are left alone and the device holds create's
 * message).  Unlike the create entry points it accepts the record-only device (CRABML_HIP_FLAG_DRY), where no kernel's LDS limit
 * can be raised: the forms that need a raise read 0 there. */
enum {
  CRABML_HIP_STEPPLAN_PATH = 0,        /* 0 per-op segments (enqueue_segment_generic), 1 the five fused launches (enqueue_segment_t),
                                          2 the K-quant fused launches (enqueue_segment_k) */
  CRABML_HIP_STEPPLAN_ORDERED = 1,     /* strict-order device: the fused launches in their block-ordered form */
  CRABML_HIP_STEPPLAN_NORM_EPI = 2,
  CRABML_HIP_STEPPLAN_NORM_EPI_K = 3,
  CRABML_HIP_STEPPLAN_DEFER_NORM = 4,
  CRABML_HIP_STEPPLAN_GU_ROWS = 5,
  CRABML_HIP_STEPPLAN_Q8K_PRODUCERS = 6,
  CRABML_HIP_STEPPLAN_K_NORM_IN = 7,
  CRABML_HIP_STEPPLAN_ATTN_LONG_OK = 8,
  CRABML_HIP_STEPPLAN_EXACT_LONG_OK = 9,
  CRABML_HIP_STEPPLAN_ATTN_LONG_FROM = 10,
  CRABML_HIP_STEPPLAN_PV_SPLIT = 11,
  CRABML_HIP_STEPPLAN_ATTN_FLASH = 12,
  CRABML_HIP_STEPPLAN_FLASH_TICKET = 13,
  CRABML_HIP_STEPPLAN_FLASH_TICKET_UNTIL = 14,
  CRABML_HIP_STEPPLAN_ATTN_FLASH_ROWS = 15,
  CRABML_HIP_STEPPLAN_FLASH_S = 16,
  CRABML_HIP_STEPPLAN_FLASH_MIN_ROWS = 17,
  CRABML_HIP_STEPPLAN_ATTN_S_ROWS = 18,
  CRABML_HIP_STEPPLAN_ATTN_S_LDS = 19,
  CRABML_HIP_STEPPLAN_USE_GRAPH = 20,  /* 1: the step is replayed from captured graphs, */
  CRABML_HIP_STEPPLAN_GRAPHS = 21,     /*   this many (one per attention variant) */
  CRABML_HIP_STEPPLAN_N_CU = 22,       /* compute units of the device */
  CRABML_HIP_STEPPLAN_WORDS = 23
};
int crabml_hip_debug_step_plan(crabml_hip_device_t* dev, const crabml_hip_llama_config_t* cfg, const crabml_hip_llama_weights_t* w,
                               const crabml_hip_llama_arch_t* arch, int32_t* words, size_t n_words);

/* ---- measurement hook (bench.py `roofline` object) -------------------------------------------------
 * While enabled, every matmul_vec GEMV kernel launch is bracketed by a pair of HIP events recorded on
 * the device's own stream (the stream the kernel runs on); crabml_hip_prof_read() drains them and
 * returns, per weight dtype, the number of launches, the summed kernel time and the summed ALGORITHMIC
 * bytes  m*(k/QK)*BLK + 4k + 4m  (SURVEY.md section 8d).  Costs one event pair per launch: use it in a
 * dedicated instrumented pass, not inside a throughput-timed region. */
typedef struct crabml_hip_prof_entry {
  uint32_t dtype;        /* weight GGML type of the GEMV */
  uint32_t reserved;     /* stage: 0 = matmul_vec; fused step (eager mode only): 1 qkv, 2 wo+res, 3 gate/up, 4 down+res, 5 classifier */
  uint64_t launches;
  double kernel_ms;      /* sum over launches of (stop - start) */
  double algo_bytes;     /* sum over launches of algorithmic bytes */
} crabml_hip_prof_entry_t;
int crabml_hip_prof_enable(crabml_hip_device_t* dev, int on);
/* blocks until the recorded events completed; fills up to cap entries, returns the count in *n */
int crabml_hip_prof_read(crabml_hip_device_t* dev, crabml_hip_prof_entry_t* out, size_t cap, size_t* n);
/* the same drain, one value per launch in record order (for medians / percentiles): fills up to cap durations in
 * milliseconds, returns the count in *n */
int crabml_hip_prof_read_launches(crabml_hip_device_t* dev, float* ms, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif /* CRABML_HIP_DEBUG_H */
