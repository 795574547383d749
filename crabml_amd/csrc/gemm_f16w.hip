// gemm_f16w.hip -- the FAST prompt pass's weight GEMM (crabml_hip_llama_prefill on the fast device; Q4_0 / Q8_0 weights x Q8_0 rows,
// Q4_1 x Q8_1, Q4_K / Q6_K / Q2_K / Q3_K x Q8_K, and -- in a context created with CRABML_HIP_LLAMA_PREFILL_Q5K_GEMM -- Q5_K x Q8_K):
// weight-stationary on the f16 matrix cores.
//
// matmul_vec with a batched rhs is `C[b, m] = W[m, k] . x[b, k]` (matmul_vec.rs:41-76: the (b, k) rhs contract; llama2.rs:111-129).
// The bit-exact form (gemm_mfma.hip: exact int8 tiles, then the reference's per-block `sumf += (sumi as f32 * d_w) * d_x`) pays
// 8-10 VALU operations per MFMA for that scaling -- it is VALU-issue-bound at 14 % MfmaUtil (profiles/r05_prefill_gemm_experiments.md).
// Here the block scales are folded into the OPERANDS and the sum runs in f32 inside the matrix core across all blocks:
//   A' = (q_w - 8) * d_w   as f16: q_w - 8 exact, ONE rounding of the product (v_pk_mul_f16)
//   B' = q_x * d_x         as f16: one rounding (k_q8_0_rows_to_f16: once per activation matrix, not per weight row tile)
//   C  = sum_k A' B'       in f32 (v_mfma_f32_16x16x32_f16), no per-block work at all.
// A deviation of the fast tier only (two extra f16 roundings per product against the reference's exact integer block dots; inside
// FAST_TOL, tests/test_hip_prefill.py); matmul_vec and the strict-order device keep the bit-exact int8 kernel.
//
// Tiling (what round 5's f16 experiment lacked): a wave owns F 16-row fragments x T = 8 column tiles of 16 prompt rows and unpacks
// each A fragment ONCE per 32 k-slots -- 15 VALU operations -- for T MFMAs: 15 F / (F T) < 2 VALU per MFMA, 0.9 with the staging
// amortized (the int8 kernel: 10.75).  A fragments come straight from global memory in MFMA layout: lane (i, g) loads the whole
// 16-byte block kb0 + g of row i (64 contiguous bytes per row and chunk) and step s = 0..3 of the chunk feeds dword s of every
// lane -- an MFMA's 32 k-slots then span FOUR blocks (8 elements of each), which the folded scales allow.  B' tiles (128 columns x
// 128 k-slots x 2 B = 32 KB per chunk) go through LDS, double-buffered, one barrier per chunk, shared by the workgroup's four waves;
// the fragment reads are conflict-free ds_read_b128 (layout: GemmF16Geo), a group of tiles ahead of the MFMAs that consume them.
//
// Q8_0 weights: the lane's block is 32 bytes (two loads); step s takes dwords s and 4 + s -- the same k-slot order as Q4_0's nibbles,
// so both formats share one B'.  A' = q_w * d_w (q_w exact).
// Q4_K weights (Q8_K rows): a chunk is HALF a super-block -- lane (i, g) loads the 16-byte class-major piece h of pair g (dword s =
// class 4 h + s: elements 8 k + 4 h + s of sub-blocks 2 g (low nibbles) and 2 g + 1 (high); common.hpp) and, once per super-block, the
// 16-byte header.  A' = n * fl16(d * sc) - fl16(dmin * m) (buf_q4_k.rs:225-263's d * sc * q - dmin * m, per element): n exact, the
// product exact inside ONE v_pk_fma_f16, so three f16 roundings per weight element; B' = q_x * d_x from the Q8_K planes in the
// matching slot order (k_rows_to_f16<1>).
// Q4_1 weights (Q8_1 rows): Q4_0's loads and slot order; A' = n * d + m in one v_pk_fma_f16 (buf_q4_1.rs: d * q + m per element --
// the rows' `s` term of the integer form is not needed).
// Q6_K weights (Q8_K rows): a chunk is one 128-element half of a super-block -- lane (i, g) loads 16 bytes of ql (g < 2: ql[0..31],
// the low nibbles are quarter 0, the high ones quarter 2; g >= 2: ql[32..63], quarters 1 and 3; buf_q6_k.rs:21-48) and the 16 bytes
// of qh that carry the same l's two high bits, and once per super-block the 16 int8 scales and d.  A' = (q - 32) * fl16(d * sc),
// q - 32 exact.  Its own B' slot order (k_rows_to_f16<2>): a Q4_K_M layer converts the rows once per order it needs.
// Q2_K / Q3_K weights (Q8_K rows): element 128 h + 32 j + l of a super-block sits in bits 2 j of qs[32 h + l] (buf_q2_k.rs:35-66,
// buf_q3_k.rs:37-84), so lane (i, g) loads the 16-byte piece g of qs (h = g >> 1, l = 16 (g & 1) .. + 16) ONCE per super-block -- with
// the ring slot of its odd chunk -- and chunk c = 0, 1 of the super-block takes shifts 2 c (slots 0-3 of a step) and 2 c + 1 (slots
// 4-7) out of dword s in step s: the c_lo / c_hi split of the Q4_K unpack with a 2-bit mask.  The scale group of shift j is
// 8 h + 2 j + (g & 1).
//   Q2_K: the eight (scale | min << 4) bytes of half h and the (d, dmin) dword ride with qs.  A' = n * fl16(d * (sc & 15)) -
//   fl16(dmin * (sc >> 4)), n = 0..3 exact, the product exact inside ONE v_pk_fma_f16: three f16 roundings, as for Q4_K.
//   Q3_K: 16 bytes of hmask (bytes 16 (g & 1) .., bit 4 h + j of byte l) and the 16-byte record (scales[12], d) ride with qs.  The
//   high bit is ORed in at bit 2 of 0x6400 | low2, the bias -1028 makes it q = low2 - (hbit ? 0 : 4) exactly; A' = q * fl16(d *
//   (sc - 32)), the 6-bit sc taken out of the record as the reference's aux[] shuffle does: two roundings.
// ONE B' slot order for both (k_rows_to_f16<3>): a Q2_K-mix layer whose attn_v is Q3_K converts the rows once.
// Q5_K weights (Q8_K rows; opt-in, see fused.hip takes_f16w): element 64 p + 32 hi + l of a super-block is nibble hi of qs[32 p + l] with
// bit 2 p + hi of qh[l] on top (buf_q5_k.rs:24-63; qs in FILE order here, not class-major like Q4_K's).  Chunk c of the super-block: lane
// (i, g) loads the 16-byte piece g & 1 of pair p = 2 (g >> 1) + c (qs + 32 p + 16 (g & 1)) -- the low nibbles of dword s are elements
// 128 (g >> 1) + 64 c + 16 (g & 1) + 4 s + k, the high ones those + 32: exactly slot order 3, so Q5_K reads the B' of Q2_K / Q3_K (a
// Q3_K_M / Q3_K_L layer converts its rows once).  The 16 bytes of qh at 16 (g & 1) and the 16-byte header (Q4_K's: d, dmin, pair-major
// fields) ride ONCE per super-block in the ring slot of its odd chunk, as Q3_K's hmask and record do (asked for with the even slot, as
// Q4_K asks for its header, the odd slot's fetch of the NEXT super-block would overwrite qh while the odd chunk still reads it).  The qh
// dword s, shifted right by 4 (g >> 1) + 2 c, has the low-nibble element's fifth bit at bit 0 of every byte and the high-nibble
// element's at bit 1; it is ORed in at bit 4 of 0x6400 | nibble, bias -1024 makes it q = nibble + 16 hbit (0..31) exactly.  A' = q *
// fl16(d * sc) - fl16(dmin * m): Q4_K's c_lo / c_hi fma with the pair's four constants made per chunk, three f16 roundings.
#include <cstdlib>
#include <type_traits>

#include "devutil.hpp"
#include "f16w_rows.hpp"
#include "kernels.hpp"

namespace crabml_hip {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef h16x2 f16x2;  // (common.hpp; named like f16x8 here)

// ---- B': the rows of a prompt pass as pre-scaled f16, in the GEMM's k-slot order: xh[col][kb][32] f16 ------------------------
// (the slot orders and the conversion of one 8-slot group: f16w_rows.hpp, shared with the row kernels that write B' themselves)
// Q8_K rows (Q4_K weights): slot group kb = 4 cc + g of chunk cc = (super-block, half h), step s = class l = 4 h + s of pair g;
// slot e: k = 0, 2, 1, 3 of sub-block 2 g (e < 4) / 2 g + 1 (e >= 4), element 8 k + l -- unpack_q4_k_f16's order
// Q6_K weights: chunk cc = (super-block, half), g, step s: element 128 half + 32 (g >> 1) + 16 (g & 1) + 4 s + k (e < 4), + 64 (e >= 4)
// Q2_K / Q3_K / Q5_K weights: chunk cc = (super-block, c), g = (h, l / 16), step s: element 128 h + 32 (2 c) + 16 (g & 1) + 4 s + k (e < 4), + 32 (e >= 4)
template <int ORDER>  // 0: Q8_0 / Q8_1 rows (block order); Q8_K rows for 1: Q4_K, 2: Q6_K, 3: Q2_K / Q3_K / Q5_K weights
__global__ __launch_bounds__(256) void k_rows_to_f16(const char* __restrict__ planes, size_t row_stride, size_t off_d, int nb,
                                                     unsigned short* __restrict__ xh, int* __restrict__ ovf) {
  const size_t col = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per (block, 8-slot group)
  if (t >= nb * 4) return;
  rows_to_f16_piece<ORDER>(planes + col * row_stride, off_d, t, xh + col * (size_t)nb * 32, ovf);
}
// planes: `rows` sets of activation planes (act_layout(act_qtype, k)); the slot order is the one the weight format w_dtype reads
int gemm_f16w_order(uint32_t w_dtype) {
  return w_dtype == CRABML_HIP_Q4_K ? 1
         : w_dtype == CRABML_HIP_Q6_K ? 2
         : (w_dtype == CRABML_HIP_Q2_K || w_dtype == CRABML_HIP_Q3_K || w_dtype == CRABML_HIP_Q5_K) ? 3
                                                                                                      : 0;
}
bool launch_rows_to_f16(hipStream_t st, uint32_t act_qtype, uint32_t w_dtype, const void* planes, size_t rows, size_t k, void* xh, int* ovf) {
  if (!gemm_f16w_covers(w_dtype, act_qtype) || (act_qtype == CRABML_HIP_Q8_K && k % 256 != 0)) return false;
  const ActLayout al = act_layout(act_qtype, k);
  const int nb = (int)(k / 32);
  const dim3 grid((unsigned)((nb * 4 + 255) / 256), (unsigned)rows);
  switch (gemm_f16w_order(w_dtype)) {
    case 0: k_rows_to_f16<0><<<grid, 256, 0, st>>>((const char*)planes, al.total, al.off_d, nb, (unsigned short*)xh, ovf); break;
    case 1: k_rows_to_f16<1><<<grid, 256, 0, st>>>((const char*)planes, al.total, al.off_d, nb, (unsigned short*)xh, ovf); break;
    case 2: k_rows_to_f16<2><<<grid, 256, 0, st>>>((const char*)planes, al.total, al.off_d, nb, (unsigned short*)xh, ovf); break;
    default: k_rows_to_f16<3><<<grid, 256, 0, st>>>((const char*)planes, al.total, al.off_d, nb, (unsigned short*)xh, ovf); break;
  }
  return true;
}

// the k pieces of a split GEMM: out[j] += part[j][0] + part[j][1] + ... in piece order (deterministic), every matrix of the launch at once
struct F16wParts {
  float* out[3];
  const float* part[3];  // matrix j's first partial; the next pieces follow pstride floats apart
  size_t end4[3];        // cumulative f32x4 counts
  size_t pstride;
  int nparts;
};
__global__ __launch_bounds__(256) void k_addn_f32(F16wParts a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.end4[2]) return;
  const int j = i < a.end4[0] ? 0 : i < a.end4[1] ? 1 : 2;
  const size_t li = i - (j == 0 ? 0 : j == 1 ? a.end4[0] : a.end4[1]);
  float* o = j == 0 ? a.out[0] : j == 1 ? a.out[1] : a.out[2];
  const float* p = j == 0 ? a.part[0] : j == 1 ? a.part[1] : a.part[2];
  f32x4 v = ((const f32x4*)o)[li];
  for (int s = 0; s < a.nparts; s++) v = v + ((const f32x4*)(p + (size_t)s * a.pstride))[li];
  ((f32x4*)o)[li] = v;
}

// one dword of a Q4_0 block (quant bytes 4 s .. 4 s + 3: low nibbles = elements 4 s .., high nibbles = 16 + 4 s ..; buf_q4_0.rs:24-33)
// -> the lane's eight f16 k-slots (q - 8) * d.  0x6400 | n is the f16 number 1024 + n; -1032 makes it n - 8 exactly.
// (x & 0x000F000F) | 0x64006400 as ONE v_and_or_b32: a VOP3 instruction takes a single scalar / literal operand, so the compiler
// splits it unless one constant sits in a VGPR -- `magic` (loop-invariant, one register)
// (BITS: the width of the field at the bottom of each 16-bit half -- 4: a nibble; 2: a Q2_K / Q3_K level)
template <int BITS = 4>
__device__ __forceinline__ unsigned and_or_magic(unsigned x, unsigned magic) {
  unsigned r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(((1u << BITS) - 1u) * 0x00010001u), "v"(magic));
  return r;
}
__device__ __forceinline__ f16x8 unpack_q4_0_f16(unsigned w, f16x2 d2, unsigned magic) {
  const f16x2 bias = {(_Float16)-1032.0f, (_Float16)-1032.0f};
  const unsigned u0 = and_or_magic(w, magic), u1 = and_or_magic(w >> 8, magic);
  const unsigned u2 = and_or_magic(w >> 4, magic), u3 = and_or_magic(w >> 12, magic);
  const f16x2 p0 = (__builtin_bit_cast(f16x2, u0) + bias) * d2, p1 = (__builtin_bit_cast(f16x2, u1) + bias) * d2;
  const f16x2 p2 = (__builtin_bit_cast(f16x2, u2) + bias) * d2, p3 = (__builtin_bit_cast(f16x2, u3) + bias) * d2;
  return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// Q8_0: the bytes of a dword as f16 (b ^ 0x80 = b + 128 unsigned; 0x6400 | u = 1024 + u; -1152 makes it b exactly), pairs (b0, b2), (b1, b3)
__device__ __forceinline__ unsigned and_or_magic8(unsigned x, unsigned magic) {
  unsigned r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(0x00FF00FFu), "v"(magic));
  return r;
}
__device__ __forceinline__ f16x8 unpack_q8_0_f16(unsigned w0, unsigned w1, f16x2 d2, unsigned magic) {
  const f16x2 bias = {(_Float16)-1152.0f, (_Float16)-1152.0f};
  const unsigned x0 = w0 ^ 0x80808080u, x1 = w1 ^ 0x80808080u;
  const unsigned u0 = and_or_magic8(x0, magic), u1 = and_or_magic8(x0 >> 8, magic);
  const unsigned u2 = and_or_magic8(x1, magic), u3 = and_or_magic8(x1 >> 8, magic);
  const f16x2 p0 = (__builtin_bit_cast(f16x2, u0) + bias) * d2, p1 = (__builtin_bit_cast(f16x2, u1) + bias) * d2;
  const f16x2 p2 = (__builtin_bit_cast(f16x2, u2) + bias) * d2, p3 = (__builtin_bit_cast(f16x2, u3) + bias) * d2;
  return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
// Q4_K: one class dword of the lane's pair; cs = {d sc_lo, -dmin m_lo, d sc_hi, -dmin m_hi}, each in both halves
struct Q4KF16Consts {
  f16x2 c_lo, o_lo, c_hi, o_hi;
};
// (BITS = 2: Q2_K -- the dword already shifted so that bits 0-1 of each byte are the chunk's first shift and bits 2-3 its second)
template <int BITS = 4>
__device__ __forceinline__ f16x8 unpack_q4_k_f16(unsigned w, const Q4KF16Consts& cs, unsigned magic) {
  const f16x2 bias = {(_Float16)-1024.0f, (_Float16)-1024.0f};
  const unsigned u0 = and_or_magic<BITS>(w, magic), u1 = and_or_magic<BITS>(w >> 8, magic);
  const unsigned u2 = and_or_magic<BITS>(w >> BITS, magic), u3 = and_or_magic<BITS>(w >> (8 + BITS), magic);
  const f16x2 p0 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u0) + bias, cs.c_lo, cs.o_lo);
  const f16x2 p1 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u1) + bias, cs.c_lo, cs.o_lo);
  const f16x2 p2 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u2) + bias, cs.c_hi, cs.o_hi);
  const f16x2 p3 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u3) + bias, cs.c_hi, cs.o_hi);
  return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
__device__ __forceinline__ Q4KF16Consts q4k_f16_consts(i32x4 hdr, int g) {
  const unsigned f = q4k_pair_field((unsigned)hdr[1], (unsigned)hdr[2], (unsigned)hdr[3], g);
  const float d = h2f((unsigned short)((unsigned)hdr[0] & 0xffffu)), dmin = h2f((unsigned short)((unsigned)hdr[0] >> 16));
  const _Float16 c_lo = (_Float16)(d * (float)(f & 63u)), c_hi = (_Float16)(d * (float)((f >> 6) & 63u));  // (11 x 6 bits: exact in f32)
  const _Float16 o_lo = (_Float16)-(dmin * (float)((f >> 12) & 63u)), o_hi = (_Float16)-(dmin * (float)(f >> 18));
  return Q4KF16Consts{f16x2{c_lo, c_lo}, f16x2{o_lo, o_lo}, f16x2{c_hi, c_hi}, f16x2{o_hi, o_hi}};
}

// Q6_K: one dword of ql and the matching dword of qh, already shifted so that bits 0-1 of each byte belong to the low nibbles' quarter
// and bits 4-5 to the high nibbles'
__device__ __forceinline__ unsigned and_or_hi2(unsigned x, unsigned acc) {
  unsigned r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(0x00300030u), "v"(acc));
  return r;
}
__device__ __forceinline__ f16x8 unpack_q6_k_f16(unsigned w, unsigned hw, f16x2 c_lo, f16x2 c_hi, unsigned magic) {
  const f16x2 bias = {(_Float16)-1056.0f, (_Float16)-1056.0f};  // 1024 + q -> q - 32
  const unsigned u0 = and_or_hi2(hw << 4, and_or_magic(w, magic)), u1 = and_or_hi2(hw >> 4, and_or_magic(w >> 8, magic));
  const unsigned u2 = and_or_hi2(hw, and_or_magic(w >> 4, magic)), u3 = and_or_hi2(hw >> 8, and_or_magic(w >> 12, magic));
  const f16x2 p0 = (__builtin_bit_cast(f16x2, u0) + bias) * c_lo, p1 = (__builtin_bit_cast(f16x2, u1) + bias) * c_lo;
  const f16x2 p2 = (__builtin_bit_cast(f16x2, u2) + bias) * c_hi, p3 = (__builtin_bit_cast(f16x2, u3) + bias) * c_hi;
  return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}


// Q2_K: unpack_q4_k_f16<2>; the constants of chunk c of the lane's piece: scale bytes 2 (2 c + u) + (g & 1), u = 0, 1, of its half's eight (sc: dword c of them)
__device__ __forceinline__ Q4KF16Consts q2k_f16_consts(unsigned sc, unsigned dm, int g) {
  const unsigned b = sc >> (8 * (g & 1));  // the two bytes at bits 0 and 16
  const float d = h2f((unsigned short)(dm & 0xffffu)), dmin = h2f((unsigned short)(dm >> 16));
  const _Float16 c_lo = (_Float16)(d * (float)(b & 15u)), c_hi = (_Float16)(d * (float)((b >> 16) & 15u));  // (11 x 4 bits: exact in f32)
  const _Float16 o_lo = (_Float16)-(dmin * (float)((b >> 4) & 15u)), o_hi = (_Float16)-(dmin * (float)((b >> 20) & 15u));
  return Q4KF16Consts{f16x2{c_lo, c_lo}, f16x2{o_lo, o_lo}, f16x2{c_hi, c_hi}, f16x2{o_hi, o_hi}};
}
// Q3_K: hw = the matching dword of hmask, already shifted so that bit 0 of each byte belongs to the first shift and bit 1 to the
// second; ORed in at bit 2 (the way and_or_hi2 does for Q6_K): 1024 + low2 + 4 hbit, -1028 makes it q = low2 - (hbit ? 0 : 4)
__device__ __forceinline__ unsigned and_or_hbit(unsigned x, unsigned acc) {
  unsigned r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(0x00040004u), "v"(acc));
  return r;
}
__device__ __forceinline__ f16x8 unpack_q3_k_f16(unsigned w, unsigned hw, f16x2 c_lo, f16x2 c_hi, unsigned magic) {
  const f16x2 bias = {(_Float16)-1028.0f, (_Float16)-1028.0f};
  const unsigned u0 = and_or_hbit(hw << 2, and_or_magic<2>(w, magic)), u1 = and_or_hbit(hw >> 6, and_or_magic<2>(w >> 8, magic));
  const unsigned u2 = and_or_hbit(hw << 1, and_or_magic<2>(w >> 2, magic)), u3 = and_or_hbit(hw >> 7, and_or_magic<2>(w >> 10, magic));
  const f16x2 p0 = (__builtin_bit_cast(f16x2, u0) + bias) * c_lo, p1 = (__builtin_bit_cast(f16x2, u1) + bias) * c_lo;
  const f16x2 p2 = (__builtin_bit_cast(f16x2, u2) + bias) * c_hi, p3 = (__builtin_bit_cast(f16x2, u3) + bias) * c_hi;
  return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
// the two constants fl16(d * (sc - 32)) of chunk c of the lane's piece: scale indices 8 h + 2 (2 c + u) + (g & 1), u = 0, 1, of the record
// (scales[12], d): index j's low nibble is nibble j / 8 of byte j % 8, its two high bits sit at bit 2 (j / 4) of byte 8 + j % 4
// (buf_q3_k.rs's aux[] shuffle)
template <int C>
__device__ __forceinline__ void q3k_f16_consts(i32x4 rec, int g, f16x2& c_lo, f16x2& c_hi) {
  const int h = g >> 1;
  const unsigned lo = (unsigned)rec[C] >> (8 * (g & 1) + 4 * h), hi = (unsigned)rec[2] >> (8 * (g & 1) + 2 * (2 * h + C));
  const int s0 = (int)((lo & 15u) | ((hi & 3u) << 4)) - 32, s1 = (int)(((lo >> 16) & 15u) | (((hi >> 16) & 3u) << 4)) - 32;
  const float d = h2f((unsigned short)((unsigned)rec[3] & 0xffffu));
  const _Float16 a = (_Float16)(d * (float)s0), b = (_Float16)(d * (float)s1);  // (11 x 6 bits: exact in f32)
  c_lo = f16x2{a, a};
  c_hi = f16x2{b, b};
}

// Q5_K: one dword of the lane's piece of qs and the matching dword of qh, already shifted so that bit 0 of each byte belongs to the low
// nibbles' sub-block and bit 1 to the high nibbles'; ORed in at bit 4: 1024 + nibble + 16 hbit, -1024 makes it q = 0..31; then Q4_K's fma
__device__ __forceinline__ unsigned and_or_bit4(unsigned x, unsigned acc) {
  unsigned r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(0x00100010u), "v"(acc));
  return r;
}
__device__ __forceinline__ f16x8 unpack_q5_k_f16(unsigned w, unsigned hw, const Q4KF16Consts& cs, unsigned magic) {
  const f16x2 bias = {(_Float16)-1024.0f, (_Float16)-1024.0f};
  const unsigned u0 = and_or_bit4(hw << 4, and_or_magic(w, magic)), u1 = and_or_bit4(hw >> 4, and_or_magic(w >> 8, magic));
  const unsigned u2 = and_or_bit4(hw << 3, and_or_magic(w >> 4, magic)), u3 = and_or_bit4(hw >> 5, and_or_magic(w >> 12, magic));
  const f16x2 p0 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u0) + bias, cs.c_lo, cs.o_lo);
  const f16x2 p1 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u1) + bias, cs.c_lo, cs.o_lo);
  const f16x2 p2 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u2) + bias, cs.c_hi, cs.o_hi);
  const f16x2 p3 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u3) + bias, cs.c_hi, cs.o_hi);
  return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// Q5_0 / Q5_1: dword s of a block's qs (elements 4 s .. 4 s + 3 in the low nibbles, 16 + 4 s .. in the high ones; buf_q5_0.rs:22-37) with
// their fifth bits -- qh bits 4 s .. 4 s + 3 (hl) and 16 + 4 s .. (hh), four bits each -- ORed in at bit 4 of 0x6400 | nibble as the
// Q5_K form does.  A slot pair holds bytes (0, 2) or (1, 3) of the dword: h << 4 | h << 18 has bit 0 of h at bit 4 and bit 2 at bit 20,
// and one position down bits 1 and 3.
__device__ __forceinline__ unsigned q5_bit4_pairs(unsigned h) { return (h << 4) | (h << 18); }
template <bool Q51>  // Q5_0: A' = (q5 - 16) * d, one f16 rounding; Q5_1: A' = q5 * d + m in one v_pk_fma_f16, one rounding
__device__ __forceinline__ f16x8 unpack_q5_01_f16(unsigned w, unsigned hl, unsigned hh, f16x2 d2, f16x2 m2, unsigned magic) {
  const _Float16 b = Q51 ? (_Float16)-1024.0f : (_Float16)-1040.0f;  // 1024 + q5 -> q5, or q5 - 16, exactly
  const f16x2 bias = {b, b};
  const unsigned xl = q5_bit4_pairs(hl), xh = q5_bit4_pairs(hh);
  const unsigned u0 = and_or_bit4(xl, and_or_magic(w, magic)), u1 = and_or_bit4(xl >> 1, and_or_magic(w >> 8, magic));
  const unsigned u2 = and_or_bit4(xh, and_or_magic(w >> 4, magic)), u3 = and_or_bit4(xh >> 1, and_or_magic(w >> 12, magic));
  f16x2 p0, p1, p2, p3;
  if constexpr (Q51) {
    p0 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u0) + bias, d2, m2);
    p1 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u1) + bias, d2, m2);
    p2 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u2) + bias, d2, m2);
    p3 = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, u3) + bias, d2, m2);
  } else {
    p0 = (__builtin_bit_cast(f16x2, u0) + bias) * d2;
    p1 = (__builtin_bit_cast(f16x2, u1) + bias) * d2;
    p2 = (__builtin_bit_cast(f16x2, u2) + bias) * d2;
    p3 = (__builtin_bit_cast(f16x2, u3) + bias) * d2;
  }
  return f16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

enum { WF_Q4_0 = 0, WF_Q8_0 = 1, WF_Q4_K = 2, WF_Q6_K = 3, WF_Q4_1 = 4, WF_Q2_K = 5, WF_Q3_K = 6, WF_Q5_K = 7, WF_Q5_0 = 8, WF_Q5_1 = 9 };  // the weight format of a GEMM
// the forms whose rows are Q8_K: a chunk is half a super-block, so k is whole super-blocks and the k pieces of a split launch start on
// super-block boundaries
constexpr bool f16w_wf_superblock(int wf) { return wf == WF_Q4_K || wf == WF_Q6_K || wf == WF_Q2_K || wf == WF_Q3_K || wf == WF_Q5_K; }

template <int T_>
struct GemmF16Geo {
  static constexpr int T = T_, CW = 16 * T;    // column tiles per wave / prompt rows per workgroup
  static constexpr int KCH = 4;                // blocks per chunk
  // An LDS buffer is [block of the chunk g][column][80 bytes]: a column's 64 bytes of one block + 16 of padding.  ds_read_b128 is
  // serviced in four 16-lane groups that mix lanes of two k-slot groups g (MI355X_MICROARCH.md, LDS: {0-3, 12-15, 20-27}, ...) over 64
  // banks: with 80-byte columns the 16 columns of a tile sit on the 16 different 16-byte slots of the 256-byte bank row (5 i mod 16),
  // and the blocks' planes are a multiple of 256 bytes apart, so every lane group is conflict-free whichever g its lanes belong to.
  static constexpr int CSTR = 80, GSTR = CW * CSTR;
  static_assert(GSTR % 256 == 0, "block planes must be whole bank rows apart");
  static constexpr int BUF = KCH * GSTR, LDS_BYTES = 2 * BUF;
  static constexpr int B_LOADS = CW * KCH * 4 / 256;  // 16-byte pieces per thread and chunk (T)
};

// Up to three weight matrices against the same rhs in ONE launch (wq | wk | wv: the 1024-row k / v GEMMs alone leave most of the
// chip idle for a whole serial k loop): row tile rt belongs to the first matrix whose cumulative tile count exceeds it.
struct F16wMats {
  const i32x4* wq[3];  // the quant plane
  const char* wd[3];   // the scale plane (f16 per block; Q4_1: (d, m); Q4_K: the 16-byte headers; Q6_K / Q5_K: the qh plane; Q2_K: the scale bytes; Q3_K: hmask)
  const char* ws2[3];  // Q6_K: the int8 scales (16 per super-block) ...; Q2_K: the (d, dmin) dwords; Q3_K: the 16-byte records; Q5_K: the 16-byte headers
  const char* ws3[3];  // ... and d (f16 per super-block)
  float* out[3];
  float* out2[3];    // ksplit > 1: k piece s >= 1 writes its partial tiles to out2[j] + (s - 1) pstride (k_addn_f32 adds them)
  size_t pstride;
  FfnAct act;                      // GU launches: the activation of h = act(g) * u and its f16 table (ffn_act_mul, devutil.hpp)
  F16wHQuant hq;                   // GU launches: h leaves as Q8_0 / Q8_1 planes (+ ffn_down's B') instead of f32 (planes == nullptr: f32)
  int m[3];
  int tiles_end[3];  // cumulative row tiles
};
// GU (F = 2, two matrices of the same shape: ffn_gate and ffn_up): fragment 0 holds 16 rows of the FIRST matrix, fragment 1 the same
// 16 rows of the SECOND -- the workgroup owns 64 rows of both -- and the epilogue stores h = silu(g) * u (out[0]) instead of g and u:
// the (rows, hidden) f32 pair never makes its trip through memory (llama2.rs:620-630).  One k piece only (silu is not linear).
template <int WF, int F, int T_, bool GU = false>  // F 16-row fragments x T_ 16-column tiles per wave: the workgroup's four waves own 64 F consecutive weight rows
// ksplit > 1: that many workgroups per output tile, each over its piece of k, each writing its own partial buffer -- ffn_down and wo
// have few row tiles and a long serial k loop (one wave per SIMD otherwise), and a short pass has few tiles altogether
__global__ __launch_bounds__(256, 2) void k_gemm_f16w(F16wMats mats, const i32x4* __restrict__ xh, int nb, int n, int row_tiles, int ksplit) {
  using G = GemmF16Geo<T_>;
  constexpr int T = G::T, KCH = G::KCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char f16w_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_in_wg();
  const int i = lane & 15, g = lane >> 4;
  int rt, ct, ks;
  {  // XCD-aware tile order (gemm_mfma.hip): the column tiles (and k halves) of a weight row tile back to back on ONE XCD
    const int per_row = (int)gridDim.x / row_tiles, col_tiles = per_row / ksplit;
    int sub;
    if ((row_tiles & 7) == 0) {
      const int x = (int)blockIdx.x & 7, j = (int)blockIdx.x >> 3;
      sub = j % per_row;
      rt = (j / per_row) * 8 + x;
    } else {
      rt = (int)blockIdx.x % row_tiles;
      sub = (int)blockIdx.x / row_tiles;
    }
    ct = sub % col_tiles;
    ks = sub / col_tiles;
  }
  static_assert(!GU || F == 2, "gate | up: one fragment of each matrix per wave");
  const int ti = GU ? 0 : rt < mats.tiles_end[0] ? 0 : rt < mats.tiles_end[1] ? 1 : 2;  // (uniform)
  // fragment f's matrix: the row tile's (ti), or -- GU -- matrix f
#define F16W_SEL(arr, j) ((j) == 0 ? mats.arr[0] : (j) == 1 ? mats.arr[1] : mats.arr[2])
#define F16W_PTRS(f)                                                                   \
  const int mj = GU ? (f) : ti;                                                        \
  const i32x4* __restrict__ wq = F16W_SEL(wq, mj);                                     \
  const char* __restrict__ wsc = F16W_SEL(wd, mj);                                     \
  const unsigned short* __restrict__ wd = (const unsigned short*)wsc;                  \
  const i32x4* __restrict__ wh = (const i32x4*)wsc;                                    \
  const i32x4* __restrict__ w6s = (const i32x4*)F16W_SEL(ws2, mj);                     \
  const unsigned short* __restrict__ w6d = (const unsigned short*)F16W_SEL(ws3, mj);   \
  (void)wq; (void)wd; (void)wh; (void)w6s; (void)w6d; (void)wsc
  float* __restrict__ out = ks == 0 ? (ti == 0 ? mats.out[0] : ti == 1 ? mats.out[1] : mats.out[2])
                                    : (ti == 0 ? mats.out2[0] : ti == 1 ? mats.out2[1] : mats.out2[2]) + (size_t)(ks - 1) * mats.pstride;
  const int m = ti == 0 ? mats.m[0] : ti == 1 ? mats.m[1] : mats.m[2];
  const int rt_l = rt - (ti == 0 ? 0 : ti == 1 ? mats.tiles_end[0] : mats.tiles_end[1]);
  constexpr int FSTEP = GU ? 0 : 16;  // rows between a wave's fragments
  const int r0 = GU ? rt_l * 64 + wave * 16 : rt_l * 64 * F + wave * 16 * F, c0 = ct * G::CW;
  // this workgroup's chunks: [ch_lo, ch_lo + nchunks) of the row's ceil(nb / KCH)
  // (Q4_K: an even chunk is half 0 of its super-block -- the pieces start on super-block boundaries)
  const int all_chunks = (nb + KCH - 1) / KCH;
  const int per_piece = f16w_wf_superblock(WF) ? (((all_chunks + ksplit - 1) / ksplit + 1) & ~1) : (all_chunks + ksplit - 1) / ksplit;
  const int ch_lo = ks * per_piece;
  const int nchunks = all_chunks - ch_lo < per_piece ? all_chunks - ch_lo : per_piece;  // (>= 1: the launcher splits only long rows)

  // A: the lane's block (row i of fragment f, block kb0 + g) and its scale.  HBM latency is several chunk times (a chunk is ~0.4 us of
  // MFMAs and a workgroup has the SIMD almost to itself): a RING of four register sets, chunk c + 3 requested while chunk c is
  // multiplied; B' (L2-resident) two chunks ahead in two register sets.  All ring indices are compile-time (chunk loop unrolled by 4).
  // (Q2_K / Q3_K: per SUPER-BLOCK, in the ring slot of its odd chunk -- the even chunk reads its neighbour's slot; the even slots stay empty)
  // (Q5_K: qs per chunk in [2 f]; qh and the header per SUPER-BLOCK in the ring slot of its odd chunk, [2 f + 1] and hq)
  constexpr int NQ = (WF == WF_Q8_0 || WF == WF_Q6_K || WF == WF_Q3_K || WF == WF_Q5_K) ? 2 : 1;  // 16-byte quant loads per fragment and chunk
  i32x4 aq[4][NQ * F];
  unsigned ad[4][F];   // Q4_0 / Q8_0 / Q5_0: the block's scale; Q4_1 / Q5_1: d | m << 16
  unsigned aqh[4][(WF == WF_Q5_0 || WF == WF_Q5_1) ? F : 1];  // Q5_0 / Q5_1: the block's qh dword, riding with its quants and scale
  i32x4 hq[2][F];      // Q4_K: the super-block header of ring slots (0, 1) / (2, 3), fetched with the even slot; Q6_K: the 16 scales
                       // Q2_K: the half's eight scale bytes ([0], [1]), fetched with the ODD slot; Q3_K: the record, Q5_K: the header, likewise
  unsigned hd[2][F];   // Q6_K: d; Q2_K: d | dmin << 16
  auto fetch_a = [&](auto Jc, int ch) {
    constexpr int J = decltype(Jc)::value;
    const int cc = ch_lo + (ch < nchunks ? ch : nchunks - 1);  // (past the end: re-read the last chunk, never consumed)
    if constexpr (WF == WF_Q4_K) {
      const int nsb = nb >> 3, sb = cc >> 1, h = cc & 1;
#pragma unroll
      for (int f = 0; f < F; f++) {
        F16W_PTRS(f);
        const int row = r0 + FSTEP * f + i;
        const size_t blk = (size_t)(row < m ? row : m - 1) * nsb + sb;
        aq[J][f] = __builtin_nontemporal_load(wq + blk * 8 + 2 * g + h);
        if constexpr ((J & 1) == 0) hq[J >> 1][f] = __builtin_nontemporal_load(wh + blk);
      }
    } else if constexpr (WF == WF_Q2_K || WF == WF_Q3_K) {
      // the super-block of chunks (ch - 1, ch), asked for with the odd one: requested while chunk ch - 3 is multiplied, first consumed
      // two chunks later, and not overwritten before chunk ch + 1 (the slot's next fetch comes with chunk ch + 1's)
      if constexpr ((J & 1) == 1) {
        const int nsb = nb >> 3, sb = cc >> 1;
#pragma unroll
        for (int f = 0; f < F; f++) {
          F16W_PTRS(f);
          const int row = r0 + FSTEP * f + i;
          const size_t blk = (size_t)(row < m ? row : m - 1) * nsb + sb;
          aq[J][NQ * f] = __builtin_nontemporal_load(wq + blk * 4 + g);
          if constexpr (WF == WF_Q3_K) {
            aq[J][NQ * f + 1] = __builtin_nontemporal_load(wh + blk * 2 + (g & 1));  // (wh: the hmask plane, 32 bytes per super-block)
            hq[J >> 1][f] = __builtin_nontemporal_load(w6s + blk);
          } else {
            const i32x2 sc = __builtin_nontemporal_load((const i32x2*)(wsc + blk * 16) + (g >> 1));
            hq[J >> 1][f] = i32x4{sc[0], sc[1], 0, 0};
            hd[J >> 1][f] = __builtin_nontemporal_load((const unsigned*)w6s + blk);
          }
        }
      }
    } else if constexpr (WF == WF_Q5_K) {
      const int nsb = nb >> 3, sb = cc >> 1, c = cc & 1;
#pragma unroll
      for (int f = 0; f < F; f++) {
        F16W_PTRS(f);
        const int row = r0 + FSTEP * f + i;
        const size_t blk = (size_t)(row < m ? row : m - 1) * nsb + sb;
        aq[J][2 * f] = __builtin_nontemporal_load(wq + blk * 8 + 4 * (g >> 1) + 2 * c + (g & 1));  // piece g & 1 of pair 2 (g >> 1) + c
        if constexpr ((J & 1) == 1) {  // the super-block of chunks (ch - 1, ch): two chunks of look-ahead, as for Q2_K / Q3_K
          aq[J][2 * f + 1] = __builtin_nontemporal_load(wh + blk * 2 + (g & 1));  // (wh: the qh plane, 32 bytes per super-block)
          hq[J >> 1][f] = __builtin_nontemporal_load(w6s + blk);
        }
      }
    } else if constexpr (WF == WF_Q6_K) {
      const int nsb = nb >> 3, sb = cc >> 1, half = cc & 1;
#pragma unroll
      for (int f = 0; f < F; f++) {
        F16W_PTRS(f);
        const int row = r0 + FSTEP * f + i;
        const size_t blk = (size_t)(row < m ? row : m - 1) * nsb + sb;
        aq[J][2 * f] = __builtin_nontemporal_load(wq + blk * 8 + 4 * half + g);
        aq[J][2 * f + 1] = __builtin_nontemporal_load(wh + blk * 4 + 2 * half + (g & 1));  // (wh: the qh plane, 64 bytes per super-block)
        if constexpr ((J & 1) == 0) {
          hq[J >> 1][f] = __builtin_nontemporal_load(w6s + blk);
          hd[J >> 1][f] = __builtin_nontemporal_load(w6d + blk);
        }
      }
    } else {
      const int kb = cc * KCH + g;
      const int gkb = kb < nb ? kb : nb - 1;
#pragma unroll
      for (int f = 0; f < F; f++) {
        F16W_PTRS(f);
        const int row = r0 + FSTEP * f + i;
        const size_t blk = (size_t)(row < m ? row : m - 1) * nb + gkb;
#pragma unroll
        for (int u = 0; u < NQ; u++) aq[J][NQ * f + u] = __builtin_nontemporal_load(wq + blk * NQ + u);
        unsigned dv;
        if constexpr (WF == WF_Q4_1) {
          dv = __builtin_nontemporal_load((const unsigned*)wsc + blk);
        } else if constexpr (WF == WF_Q5_1) {  // (d, m, qh): eight bytes per block
          const i32x2 rec = __builtin_nontemporal_load((const i32x2*)wsc + blk);
          dv = (unsigned)rec[0];
          aqh[J][f] = (unsigned)rec[1];
        } else if constexpr (WF == WF_Q5_0) {  // qh[n] u32 (wsc) | d[n] f16 (ws2)
          aqh[J][f] = __builtin_nontemporal_load((const unsigned*)wsc + blk);
          dv = __builtin_nontemporal_load((const unsigned short*)w6s + blk);
        } else {
          dv = __builtin_nontemporal_load(wd + blk);
        }
        ad[J][f] = kb < nb ? dv : 0u;  // past the row's end: scale 0 (and m 0), the slots add nothing
      }
    }
  };
  // B': 128 columns x 256 bytes per chunk, 8 pieces per thread (piece p: column p / 16, 16 bytes p % 16 of the chunk): ONE 32-bit
  // byte offset per thread, advanced by a chunk = 256 bytes per fetch (the fetches come in chunk order), against a scalar base per
  // piece -- 16 columns further each (global_load ... s[base], v offset: no per-piece pointer registers).  Columns past n (a ragged
  // last tile) and the look-ahead of the last iterations read whatever follows in xh -- launch_gemm_f16w's contract keeps that
  // inside the allocation; finite or not, it meets only output columns that are never stored, or is never consumed.  The k-slots
  // past a ragged row's end (nb % KCH != 0) read the next column's first blocks -- finite B' (a pass whose B' overflowed is computed
  // again without this GEMM: prefill_chunk) -- and, for the last column, the blocks behind it, which launch_gemm_f16w zeroes: zero
  // weights times a finite value add exactly 0 (times +-inf or NaN they would make NaN).
  // register sets of B' pieces in flight (one wave per SIMD: the longer look-ahead; the 32-byte-per-lane formats with two fragments:
  // one set -- B' is L2-resident and a chunk of 64 MFMAs per wave is longer than an L2 round trip)
  // (Q5_K with two fragments: qs per chunk AND qh + header per super-block are in flight -- one set, or F = 2, T = 8 does not fit 256 VGPRs)
  constexpr int NBD = (F == 1 && WF == WF_Q4_0) ? 4 : (F == 2 && (WF == WF_Q8_0 || WF == WF_Q6_K || WF == WF_Q5_K)) ? 1 : 2;
  i32x4 rb[NBD][G::B_LOADS];
  const char* xbase = (const char*)xh + ((size_t)c0 * nb + (size_t)ch_lo * KCH) * 64;  // (uniform)
  const unsigned xstep = 16u * (unsigned)nb * 64u;                                        // 16 columns
  unsigned xoff = (unsigned)(tid >> 4) * (unsigned)nb * 64u + (unsigned)(tid & 15) * 16u;
  auto fetch_b = [&](i32x4 (&r)[G::B_LOADS], int ch) {
    (void)ch;
#pragma unroll
    for (int u = 0; u < G::B_LOADS; u++) r[u] = *(const i32x4*)(xbase + (size_t)u * xstep + xoff);
    xoff += KCH * 64;
  };
  auto commit_b = [&](const i32x4 (&r)[G::B_LOADS], int buf) {
    unsigned char* S = f16w_lds + buf * G::BUF;
#pragma unroll
    for (int u = 0; u < G::B_LOADS; u++) {
      const int p = tid + 256 * u, col = p >> 4, pc = p & 15;
      *(i32x4*)(S + (pc >> 2) * G::GSTR + col * G::CSTR + (pc & 3) * 16) = r[u];
    }
  };

  f32x4 acc[F][T];
#pragma unroll
  for (int f = 0; f < F; f++)
#pragma unroll
    for (int t = 0; t < T; t++) acc[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  unsigned magic = 0x64006400u;
  asm volatile("" : "+v"(magic));  // pinned in a VGPR (and_or_magic)

  fetch_b(rb[0], 0);
  fetch_a(std::integral_constant<int, 0>{}, 0);
  fetch_a(std::integral_constant<int, 1>{}, 1);
  fetch_a(std::integral_constant<int, 2>{}, 2);
  Q4KF16Consts cs[F];  // Q4_K: the lane's pair's constants of the current super-block (made in the even slot); Q4_1: (d, m); Q6_K: d sc
                       // Q2_K / Q3_K / Q5_K: the constants of the current CHUNK (Q3_K: c_lo and c_hi only)
  commit_b(rb[0], 0);
  // chunk c sits in rb[c % NBD] from NBD chunks before it is committed (the fetches come in chunk order: pb advances)
#pragma unroll
  for (int c = 1; c <= NBD; c++) fetch_b(rb[c % NBD], c);
  __syncthreads();
  // chunk ch (ring slot J, LDS buffer ch & 1)
  auto chunk = [&](auto Jc, int ch) {
    constexpr int J = decltype(Jc)::value;
    fetch_a(std::integral_constant<int, (J + 3) & 3>{}, ch + 3);
    const unsigned char* S = f16w_lds + (J & 1) * G::BUF + g * G::GSTR + i * G::CSTR;
    f16x2 d2[F];
#pragma unroll
    for (int f = 0; f < F; f++) {
      if constexpr (WF == WF_Q4_K) {
        if constexpr ((J & 1) == 0) cs[f] = q4k_f16_consts(hq[J >> 1][f], g);
      } else if constexpr (WF == WF_Q6_K) {
        // the lane's two scales of a half: sc[8 half + (g & 1) + 2 (g >> 1)] (low nibbles' quarter) and 4 further (high nibbles');
        // both halves' in the even slot (the odd slot's fetch re-uses the header registers): c_* = half 0, o_* = half 1
        if constexpr ((J & 1) == 0) {
          const int sh = 8 * ((g & 1) + 2 * (g >> 1));
          const float d = h2f((unsigned short)hd[J >> 1][f]);
          _Float16 c[4];
#pragma unroll
          for (int u = 0; u < 4; u++) c[u] = (_Float16)(d * (float)(signed char)(((unsigned)hq[J >> 1][f][u] >> sh) & 0xffu));
          cs[f].c_lo = f16x2{c[0], c[0]};
          cs[f].c_hi = f16x2{c[1], c[1]};
          cs[f].o_lo = f16x2{c[2], c[2]};
          cs[f].o_hi = f16x2{c[3], c[3]};
        }
      } else if constexpr (WF == WF_Q2_K) {
        cs[f] = q2k_f16_consts((unsigned)hq[J >> 1][f][J & 1], hd[J >> 1][f], g);
      } else if constexpr (WF == WF_Q3_K) {
        q3k_f16_consts<(J & 1)>(hq[J >> 1][f], g, cs[f].c_lo, cs[f].c_hi);
      } else if constexpr (WF == WF_Q5_K) {
        cs[f] = q4k_f16_consts(hq[J >> 1][f], 2 * (g >> 1) + (J & 1));  // the chunk's pair
      } else if constexpr (WF == WF_Q4_1 || WF == WF_Q5_1) {
        const unsigned dm = ad[J][f];
        cs[f].c_lo = cs[f].c_hi = __builtin_bit_cast(f16x2, (dm & 0xffffu) | (dm << 16));
        cs[f].o_lo = cs[f].o_hi = __builtin_bit_cast(f16x2, (dm >> 16) | (dm & 0xffff0000u));
      } else {
        d2[f] = __builtin_bit_cast(f16x2, ad[J][f] | (ad[J][f] << 16));
      }
    }
    // B' fragments in groups of TG tiles, two groups in registers: group q + 1 is read from LDS while group q is multiplied (left
    // to itself the compiler reads ONE fragment, waits, multiplies: 32 exposed LDS round trips per chunk with the SIMD almost to
    // itself).  The scheduling barriers keep the reads of a group ahead of the MFMAs of the previous one.
    constexpr int TG = T >= 4 ? 4 : T, NG = 4 * (T / TG);  // groups per chunk (4 steps x T / TG)
    f16x8 bq[2][TG];
    auto read_group = [&](f16x8 (&dst)[TG], int q) {
      const int s = q / (T / TG), t0 = (q % (T / TG)) * TG;
#pragma unroll
      for (int t = 0; t < TG; t++) dst[t] = *(const f16x8*)(S + (t0 + t) * 16 * G::CSTR + s * 16);
    };
    read_group(bq[0], 0);
    f16x8 a[F];
#pragma unroll
    for (int q = 0; q < NG; q++) {
      const int s = q / (T / TG), t0 = (q % (T / TG)) * TG;
      if (q + 1 < NG) read_group(bq[(q + 1) & 1], q + 1);
      if (q % (T / TG) == 0) {
#pragma unroll
        for (int f = 0; f < F; f++) {
          if constexpr (WF == WF_Q4_0) a[f] = unpack_q4_0_f16((unsigned)aq[J][f][s], d2[f], magic);
          if constexpr (WF == WF_Q8_0) a[f] = unpack_q8_0_f16((unsigned)aq[J][2 * f][s], (unsigned)aq[J][2 * f + 1][s], d2[f], magic);
          if constexpr (WF == WF_Q4_K || WF == WF_Q4_1) a[f] = unpack_q4_k_f16((unsigned)aq[J][f][s], cs[f], magic);
          if constexpr (WF == WF_Q2_K) a[f] = unpack_q4_k_f16<2>((unsigned)aq[J | 1][f][s] >> (4 * (J & 1)), cs[f], magic);
          if constexpr (WF == WF_Q3_K)
            a[f] = unpack_q3_k_f16((unsigned)aq[J | 1][2 * f][s] >> (4 * (J & 1)), (unsigned)aq[J | 1][2 * f + 1][s] >> (4 * (g >> 1) + 2 * (J & 1)),
                                   cs[f].c_lo, cs[f].c_hi, magic);
          if constexpr (WF == WF_Q5_0)
            a[f] = unpack_q5_01_f16<false>((unsigned)aq[J][f][s], (aqh[J][f] >> (4 * s)) & 0xFu, (aqh[J][f] >> (16 + 4 * s)) & 0xFu, d2[f], d2[f], magic);
          if constexpr (WF == WF_Q5_1)
            a[f] = unpack_q5_01_f16<true>((unsigned)aq[J][f][s], (aqh[J][f] >> (4 * s)) & 0xFu, (aqh[J][f] >> (16 + 4 * s)) & 0xFu, cs[f].c_lo, cs[f].o_lo,
                                          magic);
          if constexpr (WF == WF_Q5_K)
            a[f] = unpack_q5_k_f16((unsigned)aq[J][2 * f][s], (unsigned)aq[J | 1][2 * f + 1][s] >> (4 * (g >> 1) + 2 * (J & 1)), cs[f], magic);
          if constexpr (WF == WF_Q6_K)
            a[f] = unpack_q6_k_f16((unsigned)aq[J][2 * f][s], (unsigned)aq[J][2 * f + 1][s] >> (2 * (g >> 1)), (J & 1) ? cs[f].o_lo : cs[f].c_lo,
                                   (J & 1) ? cs[f].o_hi : cs[f].c_hi, magic);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < TG; t++)
#pragma unroll
        for (int f = 0; f < F; f++) acc[f][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[f], bq[q & 1][t], acc[f][t0 + t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    commit_b(rb[(J + 1) % NBD], (J + 1) & 1);  // chunk ch + 1 into the other buffer (read last in iteration ch - 1: behind its barrier)
    fetch_b(rb[(J + 1) % NBD], ch + 1 + NBD);  // ... and the freed register set takes chunk ch + 1 + NBD
    __syncthreads();
  };
  for (int ch = 0; ch < nchunks; ch += 4) {  // (uniform conditions: every thread takes the barrier inside a chunk or none does)
    chunk(std::integral_constant<int, 0>{}, ch);
    if (ch + 1 < nchunks) chunk(std::integral_constant<int, 1>{}, ch + 1);
    if (ch + 2 < nchunks) chunk(std::integral_constant<int, 2>{}, ch + 2);
    if (ch + 3 < nchunks) chunk(std::integral_constant<int, 3>{}, ch + 3);
  }
  // D: lane (i, g) holds rows 4 g .. 4 g + 3 of column i of every tile
  if constexpr (GU) {
    if (mats.hq.planes != nullptr) {
      // h = silu(g) * u of the workgroup's 64 rows x CW columns through LDS (the B' buffers are done), then ONE THREAD per
      // (column, 32-row block) runs the row quantizer on it (q8_quant / q8_aux, devutil.hpp: buf_q8_0.rs:87-134 / buf_q8_1.rs:90-129; the
      // block maximum and the integer sum do not depend on the order) and writes the block's quants, scale, sum and -- in the slot
      // order of ffn_down's GEMM -- its 32 pre-scaled halfs: h never exists as f32 in memory
      constexpr int CS = 68;  // floats per column (64 rows + 4: 16-byte aligned columns, four banks apart)
      float* H = (float*)f16w_lds;
      __syncthreads();
#pragma unroll
      for (int t = 0; t < T; t++) {
        f32x4 hv;
#pragma unroll
        for (int r = 0; r < 4; r++) hv[r] = ffn_act_mul(acc[0][t][r], acc[1][t][r], mats.act);
        *(f32x4*)(H + (16 * t + i) * CS + wave * 16 + 4 * g) = hv;
      }
      __syncthreads();
      const F16wHQuant& hq = mats.hq;
      const int nbh = m / 32;
      for (int b = tid; b < G::CW * 2; b += 256) {
        const int col = c0 + (b >> 1), hb = rt_l * 2 + (b & 1);
        if (col >= n || hb >= nbh) continue;
        f32x4 v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = *(const f32x4*)(H + (b >> 1) * CS + 32 * (b & 1) + 4 * j);
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
          for (int r = 0; r < 4; r++) amax = fmaxf(amax, fabsf(v[j][r]));
        const float dd = amax / 127.0f;
        const unsigned short dh = f2h(dd);
        int q[32], sum = 0;
#pragma unroll
        for (int e = 0; e < 32; e++) {
          const float x = v[e >> 2][e & 3];
          q[e] = hq.q81 ? q8_quant<true>(x, dd) : q8_quant<false>(x, dd);
          sum += q[e];
        }
        char* p = hq.planes + (size_t)col * hq.stride;
        i32x4 pk[2];
#pragma unroll
        for (int e = 0; e < 8; e++) pk[e >> 2][e & 3] = (int)pack_q8x4(q[4 * e], q[4 * e + 1], q[4 * e + 2], q[4 * e + 3]);
        ((i32x4*)(p + (size_t)hb * 32))[0] = pk[0];
        ((i32x4*)(p + (size_t)hb * 32))[1] = pk[1];
        ((unsigned short*)(p + hq.off_d))[hb] = dh;
        if (hq.q81)
          ((unsigned short*)(p + hq.off_aux))[hb] = (unsigned short)q8_aux<true>(sum, dd);
        else
          ((int*)(p + hq.off_aux))[hb] = q8_aux<false>(sum, dd);
        if (hq.xh != nullptr) {
          const float ds = h2f(dh);
          unsigned short* xr = hq.xh + ((size_t)col * nbh + hb) * 32;
          bool inf = false;
#pragma unroll
          for (int s4 = 0; s4 < 4; s4++) {
            unsigned short o[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
              o[e] = f16w_value(q[f16w_slot_elem(8 * s4 + e)], ds);
              inf |= f16w_is_inf(o[e]);
            }
            *(i32x4*)(xr + 8 * s4) = i32x4{(int)(o[0] | ((unsigned)o[1] << 16)), (int)(o[2] | ((unsigned)o[3] << 16)),
                                           (int)(o[4] | ((unsigned)o[5] << 16)), (int)(o[6] | ((unsigned)o[7] << 16))};
          }
          f16w_flag(inf, hq.ovf);
        }
      }
      return;
    }
#pragma unroll
    for (int t = 0; t < T; t++) {
      const int col = c0 + 16 * t + i;
      if (col >= n) continue;
      const int row = r0 + 4 * g;
      f32x4 hv;
#pragma unroll
      for (int r = 0; r < 4; r++) hv[r] = ffn_act_mul(acc[0][t][r], acc[1][t][r], mats.act);
      float* o = out + (size_t)col * m + row;
      if (row + 3 < m) {
        *(f32x4*)o = hv;
      } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (row + r < m) o[r] = hv[r];
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < T; t++) {
    const int col = c0 + 16 * t + i;
    if (col >= n) continue;
#pragma unroll
    for (int f = 0; f < F; f++) {
      const int row = r0 + 16 * f + 4 * g;
      float* o = out + (size_t)col * m + row;
      if (row + 3 < m) {
        *(f32x4*)o = acc[f][t];
      } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (row + r < m) o[r] = acc[f][t][r];
      }
    }
  }
}

#undef F16W_PTRS
#undef F16W_SEL

// hipFuncAttributeMaxDynamicSharedMemorySize, once per (device, kernel)
static bool f16w_raise_lds(const crabml_hip_device* dev, const void* fn, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> have;
  std::lock_guard<std::mutex> g(mu);
  int& cur = have[{dev->ordinal, fn}];
  if (bytes <= cur) return true;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
  cur = bytes;
  return true;
}
// xh: the rows' pre-scaled f16 planes (launch_rows_to_f16) inside an allocation of gemm_f16w_xh_bytes(b, k): the kernel reads whole
// 128-column tiles and up to three chunks past the last column's end; returns false when the shape is not covered
template <int WF, int F, int T, bool GU = false>
static bool launch_f16w_t(crabml_hip_device* dev, const F16wMats& mats, int row_tiles, size_t k, const void* xh, size_t b, int ksplit) {
  using G = GemmF16Geo<T>;
  if (!f16w_raise_lds(dev, (const void*)k_gemm_f16w<WF, F, T, GU>, G::LDS_BYTES)) {  // (80 KB of dynamic LDS: raised once per device)
    (void)hipGetLastError();
    return false;
  }
  const int col_tiles = (int)((b + G::CW - 1) / G::CW);
  k_gemm_f16w<WF, F, T, GU><<<dim3(row_tiles * col_tiles * ksplit), 256, G::LDS_BYTES, dev->stream>>>(mats, (const i32x4*)xh, (int)(k / 32), (int)b,
                                                                                          row_tiles, ksplit);
  return true;
}
size_t gemm_f16w_xh_bytes(size_t rows, size_t k) { return ((rows + 127) / 128 * 128) * k * 2 + 4096; }

// A' range: 1 in *bad when some block's scales can put an |A'| above 65504 (f16: +-inf, and inf times a zero B' slot is NaN) -- the
// largest quant magnitude of the format times the block's scale, as the kernel rounds it (Q4_K: the largest 6-bit scale and minimum,
// 63; Q6_K: the super-block's own int8 scales; Q2_K: n c1 - c2 with the largest 4-bit scale and minimum, 15, and n <= 3; Q3_K: q c with
// |sc - 32| <= 32 and |q| <= 4; Q5_K: Q4_K's with q <= 31); a non-finite scale counts as out of range
__global__ __launch_bounds__(256) void k_f16w_range(const char* __restrict__ sc, const signed char* __restrict__ sc6,
                                                    const unsigned short* __restrict__ d6, size_t nblk, int wf, int* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nblk) return;
  float a = 0.0f;
  if (wf == WF_Q4_0 || wf == WF_Q8_0) {
    a = (wf == WF_Q4_0 ? 8.0f : 128.0f) * fabsf(h2f(((const unsigned short*)sc)[i]));  // |q - 8| <= 8, |q| <= 128: exact products
  } else if (wf == WF_Q4_1) {
    const unsigned dm = ((const unsigned*)sc)[i];
    a = 15.0f * fabsf(h2f((unsigned short)(dm & 0xffffu))) + fabsf(h2f((unsigned short)(dm >> 16)));  // n d + m, n <= 15
  } else if (wf == WF_Q5_0) {
    a = 16.0f * fabsf(h2f(((const unsigned short*)(sc + nblk * 4))[i]));  // (d follows qh) |q5 - 16| <= 16: an exact product
  } else if (wf == WF_Q5_1) {
    // q d + m is linear in q = 0 .. 31: the ends, as the kernel rounds them (31 d is exact in f32; one rounding to f16)
    const unsigned dm = ((const unsigned*)sc)[2 * i];
    const float d = h2f((unsigned short)(dm & 0xffffu)), m = h2f((unsigned short)(dm >> 16));
    const float top = fabsf(h2f(f2h(fmaf(31.0f, d, m))));
    a = fabsf(m) > top ? fabsf(m) : top;
    if (!(fabsf(d) <= 65504.0f) || !(fabsf(m) <= 65504.0f) || !(top <= 65504.0f)) a = __builtin_inff();  // (a non-finite field: out of range)
  } else if (wf == WF_Q4_K) {
    const unsigned h = ((const unsigned*)sc)[4 * i];
    const float c1 = h2f(f2h(63.0f * h2f((unsigned short)(h & 0xffffu)))), c2 = h2f(f2h(63.0f * h2f((unsigned short)(h >> 16))));
    a = 15.0f * fabsf(c1) + fabsf(c2);  // n c1 - c2, n <= 15
  } else if (wf == WF_Q5_K) {
    const unsigned h = ((const unsigned*)(sc + nblk * 32))[4 * i];  // (the headers follow qh)
    const float c1 = h2f(f2h(63.0f * h2f((unsigned short)(h & 0xffffu)))), c2 = h2f(f2h(63.0f * h2f((unsigned short)(h >> 16))));
    a = 31.0f * fabsf(c1) + fabsf(c2);  // q c1 - c2, q <= 31
  } else if (wf == WF_Q2_K) {
    const unsigned h = ((const unsigned*)(sc + nblk * 16))[i];  // (the (d, dmin) dwords follow the scale bytes)
    const float c1 = h2f(f2h(15.0f * h2f((unsigned short)(h & 0xffffu)))), c2 = h2f(f2h(15.0f * h2f((unsigned short)(h >> 16))));
    a = 3.0f * fabsf(c1) + fabsf(c2);
  } else if (wf == WF_Q3_K) {
    const unsigned short dh = ((const unsigned short*)(sc + nblk * 32))[8 * i + 6];  // (the records follow hmask; d behind scales[12])
    a = 4.0f * fabsf(h2f(f2h(32.0f * h2f(dh))));
  } else {
    const float d = h2f(d6[i]);
    for (int j = 0; j < 16; j++) a = fmaxf(a, 32.0f * fabsf(h2f(f2h(d * (float)sc6[16 * i + j]))));  // (q - 32) c, |q - 32| <= 32
    if (!(fabsf(d) <= 65504.0f)) a = d;
  }
  if (!(a <= 65504.0f)) *bad = 1;
}
static int f16w_wf(uint32_t dt) {
  switch (dt) {
    case CRABML_HIP_Q8_0: return WF_Q8_0;
    case CRABML_HIP_Q4_K: return WF_Q4_K;
    case CRABML_HIP_Q6_K: return WF_Q6_K;
    case CRABML_HIP_Q4_1: return WF_Q4_1;
    case CRABML_HIP_Q2_K: return WF_Q2_K;
    case CRABML_HIP_Q3_K: return WF_Q3_K;
    case CRABML_HIP_Q5_K: return WF_Q5_K;
    case CRABML_HIP_Q5_0: return WF_Q5_0;
    case CRABML_HIP_Q5_1: return WF_Q5_1;
    default: return WF_Q4_0;
  }
}
// once per weight buffer (and per version of its contents): one reduction over the scale plane, read back -- blocks the stream the
// first time (a fast-device model context asks for every matrix when it is created)
static bool f16w_range_ok(crabml_hip_device* dev, const crabml_hip_buf* w) {
  if (w->f16w_range_ver == w->version) return w->f16w_range_ok;
  void* d = nullptr;
  size_t cap = 0;
  if (pool_alloc(dev, 16, &d, &cap) != 0) return false;
  const char* base = (const char*)w->ptr + w->wl.off_scale;
  const size_t nblk = w->wl.n_blocks;
  int bad = 1;
  hipError_t e = hipMemsetAsync(d, 0, 4, dev->stream);
  if (e == hipSuccess && nblk > 0)
    k_f16w_range<<<(unsigned)((nblk + 255) / 256), 256, 0, dev->stream>>>(base, (const signed char*)(base + nblk * 64),
                                                                          (const unsigned short*)(base + nblk * 80), nblk,
                                                                          f16w_wf(w->dtype), (int*)d);
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, d, 4, hipMemcpyDeviceToHost, dev->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
  pool_free(dev, d, cap);
  if (e != hipSuccess) return false;
  w->f16w_range_ok = bad == 0;
  w->f16w_range_ver = w->version;
  return w->f16w_range_ok;
}
bool gemm_f16w_takes(crabml_hip_device* dev, const crabml_hip_buf* w, uint32_t act_qtype) {
  return gemm_f16w_covers(w->dtype, act_qtype) && f16w_range_ok(dev, w);
}
// the weight formats the kernel covers, and the rows' format each pairs with (CpuTensorBuf::quantize's choice: buf/api.rs:142-159)
bool gemm_f16w_covers(uint32_t w_dtype, uint32_t act_qtype) {
  if (act_qtype == CRABML_HIP_Q8_0) return w_dtype == CRABML_HIP_Q4_0 || w_dtype == CRABML_HIP_Q8_0 || w_dtype == CRABML_HIP_Q5_0;
  if (act_qtype == CRABML_HIP_Q8_1) return w_dtype == CRABML_HIP_Q4_1 || w_dtype == CRABML_HIP_Q5_1;
  return act_qtype == CRABML_HIP_Q8_K &&
         (w_dtype == CRABML_HIP_Q4_K || w_dtype == CRABML_HIP_Q6_K || w_dtype == CRABML_HIP_Q2_K || w_dtype == CRABML_HIP_Q3_K ||
          w_dtype == CRABML_HIP_Q5_K);
}
// wave tile: T column tiles of 16 prompt rows -- 8 (128-row workgroup tiles) from 65 rows up; short passes (a short prompt, the ragged
// tail of a long one) take 4 / 2: the MFMAs of an empty column tile cost what a full one's do
static int f16w_col_tiles_per_wave(size_t b, int variant) { return (variant & 512) ? 4 : (variant & 16) ? 8 : b <= 32 ? 2 : b <= 64 ? 4 : 8; }
template <int WF>
static bool launch_f16w_fmt(crabml_hip_device* dev, const F16wMats& mats, int row_tiles, size_t k, const void* xh, size_t b, int ksplit, int F,
                            int variant, bool gu, int T) {
  if (gu) {
    switch (T) {
      case 2: return launch_f16w_t<WF, 2, 2, true>(dev, mats, row_tiles, k, xh, b, 1);
      case 4: return launch_f16w_t<WF, 2, 4, true>(dev, mats, row_tiles, k, xh, b, 1);
      default: return launch_f16w_t<WF, 2, 8, true>(dev, mats, row_tiles, k, xh, b, 1);
    }
  }
  switch (T) {
    case 2: return F == 2 ? launch_f16w_t<WF, 2, 2>(dev, mats, row_tiles, k, xh, b, ksplit) : launch_f16w_t<WF, 1, 2>(dev, mats, row_tiles, k, xh, b, ksplit);
    case 4: return F == 2 ? launch_f16w_t<WF, 2, 4>(dev, mats, row_tiles, k, xh, b, ksplit) : launch_f16w_t<WF, 1, 4>(dev, mats, row_tiles, k, xh, b, ksplit);
    default: return F == 2 ? launch_f16w_t<WF, 2, 8>(dev, mats, row_tiles, k, xh, b, ksplit) : launch_f16w_t<WF, 1, 8>(dev, mats, row_tiles, k, xh, b, ksplit);
  }
}
// nw weight matrices (one format, the same k) against the same rhs rows: out[j] (b, m[j]) = W[j] . x
// ws (nullable), ws_floats: scratch for split launches.  When the output tiles alone leave the chip underfilled -- wo / ffn_down (few
// row tiles, a long k), any short pass -- the k range is cut into 2 / 4 / 8 pieces, one workgroup each: piece 0 writes out, the
// others their own partial buffers in ws, and k_addn_f32 adds them in piece order.  (Measured and not kept: the pieces added with
// f32 atomics onto a zeroed output -- 32.4k -> 30.1k prompt tok/s, and the sum's order would vary from run to run.)
bool launch_gemm_f16w(crabml_hip_device* dev, const crabml_hip_buf* const* w, const size_t* m, int nw, size_t k, void* xh, size_t b,
                      float* const* out, float* ws, size_t ws_floats, const FfnAct* gu_act, int* gu_done, int* defer_parts,
                      const F16wHQuant* hq, F16wForce* force) {
  if (gu_done) *gu_done = 0;
  if (defer_parts) *defer_parts = 0;
  if (nw < 1 || nw > 3 || k % 32 != 0 || b < 16) return false;
  const uint32_t dt = w[0]->dtype;
  if (!gemm_f16w_covers(dt, vec_dot_rhs_dtype(dt))) return false;  // (the one format list)
  const bool superblock = f16w_wf_superblock(f16w_wf(dt));
  if (superblock && k % 256 != 0) return false;
  for (int j = 0; j < nw; j++)
    if (w[j]->dtype != dt || m[j] % 4 != 0 || !f16w_range_ok(dev, w[j])) return false;
  static const int variant = [] {  // lab hook (CRABML_HIP_TEST_HOOKS=1 CRABML_HIP_F16W=n): 1 = two fragments, 3 = one; +8 = never split k; +16 = T = 8 always; +32 = k pieces of >= 8 chunks; +64 = no gate | up epilogue; +512 = T = 4 always; +1024 = narrow launches as <2, 4>
    const char* e = test_hook("CRABML_HIP_F16W");
    return e ? atoi(e) : 0;
  }();
  size_t mtot = 0;
  for (int j = 0; j < nw; j++) mtot += m[j];
  int T = f16w_col_tiles_per_wave(b, variant);
  if (force && force->T > 0) {
    if (force->T != 2 && force->T != 4 && force->T != 8) return false;
    T = force->T;
  }
  size_t cw = 16 * (size_t)T, col128 = (b + cw - 1) / cw;  // (column tiles of the launch)
  // two fragments per wave (every B' fragment read from LDS feeds two MFMAs) when 128-row tiles still cover the chip
  int F = ((mtot + 127) / 128) * col128 >= (size_t)dev->n_cu ? 2 : 1;
  if ((variant & 1024) && F == 1 && T == 8 && b >= 128) {  // lab: narrow launches as two fragments x four column tiles
    F = 2;
    T = 4;
    cw = 64;
    col128 = (b + cw - 1) / cw;
  }
  if ((variant & 7) == 1) F = 2;
  if ((variant & 7) == 3) F = 1;
  if (force && force->F > 0) {
    if (force->F != 1 && force->F != 2) return false;
    F = force->F;
  }
  // gate | up with the SiLU * mul epilogue (out[0] = h, out[1] untouched): when 64-row tiles of both matrices cover the chip without
  // cutting k
  const bool gu_ok = gu_act != nullptr && gu_done != nullptr && nw == 2 && m[0] == m[1];
  bool gu = gu_ok && !(variant & 64) && ((m[0] + 63) / 64) * col128 * 2 >= (size_t)dev->n_cu * 3;
  if (force && force->gu >= 0) {
    if (force->gu > 0 && !gu_ok) return false;
    gu = force->gu > 0;
  }
  if (gu) F = 2;
  F16wMats mats{};
  mats.act = gu_act ? *gu_act : FfnAct{nullptr, 0};
  const bool hquant = gu && hq != nullptr && hq->planes != nullptr && m[0] % 32 == 0;
  if (hquant) mats.hq = *hq;
  F16wParts parts{};
  int row_tiles = 0;
  size_t before = 0;  // output elements of the matrices before j
  for (int j = 0; j < 3; j++) {
    const int jj = j < nw ? j : nw - 1;
    const char* wp = (const char*)w[jj]->ptr;
    mats.wq[j] = (const i32x4*)wp;
    mats.wd[j] = wp + w[jj]->wl.off_scale;
    // (Q5_0: qs | qh | d; Q6_K: ql | qh | scales | d; Q2_K: qs | scales | (d, dmin); Q3_K: qs | hmask | records; Q5_K: qs | qh | headers, common.hpp)
    mats.ws2[j] = wp + w[jj]->wl.off_scale +
                  w[jj]->wl.n_blocks * (dt == CRABML_HIP_Q5_0 ? 4 : dt == CRABML_HIP_Q2_K ? 16 : (dt == CRABML_HIP_Q3_K || dt == CRABML_HIP_Q5_K) ? 32 : 64);
    mats.ws3[j] = wp + w[jj]->wl.off_scale + w[jj]->wl.n_blocks * 80;
    mats.out[j] = out[jj];
    mats.out2[j] = ws + before;
    mats.m[j] = (int)m[jj];
    parts.out[j] = out[jj];
    parts.part[j] = ws + before;
    if (j < nw) {
      if (!gu) row_tiles += (int)((m[j] + 64 * F - 1) / (64 * F));
      before += b * m[j];
    }
    if (gu) row_tiles = (int)((m[0] + 63) / 64);
    mats.tiles_end[j] = row_tiles;
    parts.end4[j] = before / 4;
  }
  mats.pstride = parts.pstride = before;
  // pieces of k: double while the launch is short of ~1.5 workgroups per CU, every piece keeps >= 4 chunks (and whole super-blocks),
  // and the partial buffers fit the scratch
  int ksplit = 1;
  const size_t chunks = (k + 127) / 128;
  if (ws != nullptr && !(variant & 8) && k % 128 == 0 && !gu)
    while (ksplit < 8 && (size_t)row_tiles * col128 * ksplit < (size_t)dev->n_cu * 3 / 2 && chunks % (size_t)(4 * ksplit) == 0 &&
           chunks / (size_t)(2 * ksplit) >= (size_t)((variant & 32) ? 8 : 4) && (size_t)(2 * ksplit - 1) * before <= ws_floats)
      ksplit *= 2;
  if (force && force->ksplit > 0) {  // every piece must hold at least one chunk (the kernel's per_piece), the partials must fit ws
    const int ks = force->ksplit, all_chunks = (int)((k / 32 + 3) / 4);
    const int per_piece = superblock ? (((all_chunks + ks - 1) / ks + 1) & ~1) : (all_chunks + ks - 1) / ks;
    if ((ks != 1 && ks != 2 && ks != 4 && ks != 8) || (ks > 1 && (gu || ws == nullptr || (size_t)(ks - 1) * before > ws_floats)) ||
        (ks - 1) * per_piece >= all_chunks)
      return false;
    ksplit = ks;
  }
  if (force) {
    force->used_F = F;
    force->used_T = T;
    force->used_ksplit = ksplit;
    force->used_gu = gu ? 1 : 0;
  }
  // the last column's slots past the row's end read the blocks behind it: zeros, whatever a longer pass (or anything else) left there
  const size_t nb = k / 32, pad = (nb + 3) / 4 * 4 - nb;
  if (pad != 0 && hipMemsetAsync((char*)xh + b * k * 2, 0, pad * 64, dev->stream) != hipSuccess) return false;
  bool ok;
  if (dt == CRABML_HIP_Q8_0)
    ok = launch_f16w_fmt<WF_Q8_0>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q4_K)
    ok = launch_f16w_fmt<WF_Q4_K>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q6_K)
    ok = launch_f16w_fmt<WF_Q6_K>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q4_1)
    ok = launch_f16w_fmt<WF_Q4_1>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q2_K)
    ok = launch_f16w_fmt<WF_Q2_K>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q3_K)
    ok = launch_f16w_fmt<WF_Q3_K>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q5_K)
    ok = launch_f16w_fmt<WF_Q5_K>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q5_0)
    ok = launch_f16w_fmt<WF_Q5_0>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else if (dt == CRABML_HIP_Q5_1)
    ok = launch_f16w_fmt<WF_Q5_1>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  else
    ok = launch_f16w_fmt<WF_Q4_0>(dev, mats, row_tiles, k, xh, b, ksplit, F, variant, gu, T);
  if (ok && gu) *gu_done = hquant ? 2 : 1;
  if (ok && ksplit > 1 && defer_parts != nullptr && nw == 1) {
    *defer_parts = ksplit - 1;  // the caller's next row kernel adds the pieces (ws + s * b * m, s = 0 ..) in the same order
  } else if (ok && ksplit > 1) {
    parts.nparts = ksplit - 1;
    k_addn_f32<<<(unsigned)((parts.end4[2] + 255) / 256), 256, 0, dev->stream>>>(parts);
  }
  return ok;
}

}  // namespace crabml_hip
