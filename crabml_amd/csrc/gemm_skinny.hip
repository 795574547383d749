// gemm_skinny.hip -- the fast prompt pass's weight GEMM for 2..15 activation rows: every weight byte is streamed once.
// k_gemm_skinny: Q4_0 / Q8_0 weights x Q8_0 rows (below); k_gemm_skinny_k: Q4_K / Q6_K weights x Q8_K rows (further down).
//
// Below 16 rows the prompt pass used to run the one-row GEMV once per row, i.e. it read every weight matrix b times.  k_gemm_mfma
// (gemm_mfma.hip) cannot take these passes: its 64-row workgroup tile leaves 64 workgroups at m = 4096 and its scalar-order sum forbids
// cutting k.  This kernel is shaped for the other end: a workgroup owns ONE 16-row tile of the weights and its 4 / 8 / 16 waves cut the
// row's blocks between them (k-split inside the workgroup); the launcher takes as many waves per tile as it needs to put two waves on
// every SIMD (m = 1024: 16 waves, m = 4096: 8, m >= 8192: 4), so no k-split across workgroups and no second launch is needed.
// Measured (profiles/skinny_gemm.md; Llama-3-8B shapes, Q4_0, 8 rows at depth 0): a target of 2 waves per SIMD gives 1.51 ms per
// 8-layer pass, 4 waves 1.62 ms, 8 waves 1.76 ms -- more, shorter runs per tile lose.  A gate / up launch (m = 14336) reaches 1.05 TB/s
// (Q4_K: 1.58), far from the GEMV's 5 TB/s.  Not measured: whether __launch_bounds__(1024), which also caps the 256- and 512-thread
// launches at 128 VGPRs, is what keeps a wave at two units in flight -- instantiating on the wave count with a deeper register ring is
// the next step.  The kernel takes 2..15 rows; the prompt pass
// sends it 6..15, over Q8_K rows 6..14 (at 2 and 3 rows one GEMV per row is faster, at 4 the two overlap, and the existing launch pins hold 5-row passes, and 15-row passes over Q8_K rows, to the row GEMV).
// The per-wave 16 x 16 f32 tiles are summed through LDS in wave order: a launch is deterministic, but the sum over blocks is
// re-associated against the GEMV's -- the fast tier's stated deviation, never taken by matmul_vec or the strict device.
//
// Operands.  v_mfma_i32_16x16x32_i8 with the ROLES SWAPPED against gemm_mfma.hip: operand A = the activation rows (lane l supplies 8
// k-slots of batch row l & 15, clamped to row b - 1: rows past the live ones are never read), operand B = the weights (lane l supplies
// the same k-slots of weight row l & 15, clamped to m - 1).  D then has lane l holding batch rows 4 (l >> 4) + r, r = 0..3, of weight
// row l & 15: a lane needs ONE weight scale per block -- that of the row whose quants it loads -- and the stores of a batch row are 16
// consecutive floats.
//
// Weights go HBM -> registers -> MFMA operand, no LDS.  A wave walks its run of blocks in units of 4 blocks: lane (x, g) requests
// block kb0 + g of row x as whole 16-byte vectors (a row's 4 blocks are 64 / 128 contiguous bytes), which leaves lane group g with
// all 32 k-slots of ONE block where the MFMA wants 8 k-slots of EACH block per lane group.  The 4 x 4 exchange between register index
// and lane group is two rounds of gfx950's lane swaps (v_permlane32_swap: index bit 1 <-> group bit 1, v_permlane16_swap: bit 0 <->
// bit 0), 4 VALU instructions per 4 dwords.  After it register t of lane group g holds dword g (and, for 32-byte blocks, register
// 4 + t dword 4 + g) of block kb0 + t: k-slots = the block's bytes [4g, 4g + 4) and [16 + 4g, 16 + 4g + 4), for Q4_0 the low / high
// nibbles of quant bytes [4g, 4g + 4), which are exactly the elements 4g.. and 16 + 4g.. (buf_q4_0.rs:24-33).  The product is invariant
// under a permutation of k-slots applied to both operands, so the activation rows take the same path.
// Two units are in flight per wave; block indices past the end are clamped (re-read, never multiplied), so every iteration issues the
// same loads and the compiler's s_waitcnt counts stay exact.
//
// Per block: sumf = fma(sumi as f32 * d_w, d_x, sumf), k_gemm_mfma<.., FMA = true>'s block term.
#include "devutil.hpp"
#include "kernels.hpp"

namespace crabml_hip {

struct SkinnyGeo {
  static constexpr int ROWS = 16;      // weight rows per workgroup: one MFMA tile
  static constexpr int UNIT = 4;       // blocks per unit (one per lane group)
  static constexpr int MAX_WAVES = 16;
};

// 4 x 4 exchange of (register index, lane group): afterwards register t of group g holds what register g of group t held
__device__ __forceinline__ void lane_group_transpose(unsigned& r0, unsigned& r1, unsigned& r2, unsigned& r3) {
  auto s = __builtin_amdgcn_permlane32_swap(r0, r2, false, false);
  r0 = s[0], r2 = s[1];
  s = __builtin_amdgcn_permlane32_swap(r1, r3, false, false);
  r1 = s[0], r3 = s[1];
  s = __builtin_amdgcn_permlane16_swap(r0, r1, false, false);
  r0 = s[0], r1 = s[1];
  s = __builtin_amdgcn_permlane16_swap(r2, r3, false, false);
  r2 = s[0], r3 = s[1];
}

template <int FMT>  // CRABML_HIP_Q4_0 | CRABML_HIP_Q8_0 weights x Q8_0 rows
__global__ __launch_bounds__(1024) void k_gemm_skinny(const i32x4* __restrict__ wq, const unsigned short* __restrict__ wd,
                                                      const char* __restrict__ act, size_t act_stride, size_t off_d,
                                                      float* __restrict__ out, int m, int nb, int b) {
  constexpr int AP = FMT == CRABML_HIP_Q4_0 ? 1 : 2;  // 16-byte pieces per weight block
  __shared__ float red[SkinnyGeo::MAX_WAVES * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6;
  const int x = lane & 15, g = lane >> 4;
  const int r0 = (int)blockIdx.x * SkinnyGeo::ROWS;
  const int wrow = r0 + x < m ? r0 + x : m - 1;
  const int acol = x < b ? x : b - 1;
  const i32x4* wrp = wq + (size_t)wrow * nb * AP;
  const unsigned short* wdp = wd + (size_t)wrow * nb;
  const i32x4* aqp = (const i32x4*)(act + (size_t)acol * act_stride);
  const char* adp[4];  // the scale planes of the four batch rows this lane accumulates
#pragma unroll
  for (int r = 0; r < 4; r++) adp[r] = act + (size_t)(4 * g + r < b ? 4 * g + r : b - 1) * act_stride + off_d;

  const int nunits = (nb + SkinnyGeo::UNIT - 1) / SkinnyGeo::UNIT, per = (nunits + nw - 1) / nw;
  const int u_lo = wave * per, u_hi = u_lo + per < nunits ? u_lo + per : nunits;

  struct Stage {
    i32x4 a[AP], q[2];
    unsigned short dw[4];
    unsigned long long dx[4];  // four f16 scales: blocks kb0 .. kb0 + 3 of one batch row (the plane is padded to 256 bytes)
  };
  Stage stg[2];
  auto fetch = [&](Stage& s, int u) {
    const int kb0 = u * SkinnyGeo::UNIT, kb = kb0 + g < nb ? kb0 + g : nb - 1;
#pragma unroll
    for (int p = 0; p < AP; p++) s.a[p] = __builtin_nontemporal_load(wrp + (size_t)kb * AP + p);
#pragma unroll
    for (int p = 0; p < 2; p++) s.q[p] = aqp[(size_t)kb * 2 + p];
#pragma unroll
    for (int t = 0; t < 4; t++) s.dw[t] = wdp[kb0 + t < nb ? kb0 + t : nb - 1];
#pragma unroll
    for (int r = 0; r < 4; r++) s.dx[r] = *(const unsigned long long*)(adp[r] + (size_t)kb0 * 2);
  };
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  auto multiply = [&](Stage& s, int u) {
    const int kb0 = u * SkinnyGeo::UNIT;
    unsigned ql[4] = {(unsigned)s.q[0][0], (unsigned)s.q[0][1], (unsigned)s.q[0][2], (unsigned)s.q[0][3]};
    unsigned qh[4] = {(unsigned)s.q[1][0], (unsigned)s.q[1][1], (unsigned)s.q[1][2], (unsigned)s.q[1][3]};
    lane_group_transpose(ql[0], ql[1], ql[2], ql[3]);
    lane_group_transpose(qh[0], qh[1], qh[2], qh[3]);
    unsigned wl[4] = {(unsigned)s.a[0][0], (unsigned)s.a[0][1], (unsigned)s.a[0][2], (unsigned)s.a[0][3]};
    unsigned wh[4] = {0u, 0u, 0u, 0u};
    lane_group_transpose(wl[0], wl[1], wl[2], wl[3]);
    if constexpr (AP == 2) {
#pragma unroll
      for (int d = 0; d < 4; d++) wh[d] = (unsigned)s.a[AP - 1][d];
      lane_group_transpose(wh[0], wh[1], wh[2], wh[3]);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
      if (kb0 + t >= nb) break;  // (wave-uniform) the clamped tail of the last unit
      unsigned lo, hi;
      if constexpr (FMT == CRABML_HIP_Q4_0) {
        // nibbles to signed bytes v - 8 without carries between bytes (as k_gemm_mfma does): the MFMA sums (q - 8) * x directly
        lo = (((wl[t] & 0x0F0F0F0Fu) | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
        hi = ((((wl[t] >> 4) & 0x0F0F0F0Fu) | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
      } else {
        lo = wl[t];
        hi = wh[t];
      }
      const long W = (long)(((unsigned long long)hi << 32) | (unsigned long long)lo);
      const long X = (long)(((unsigned long long)qh[t] << 32) | (unsigned long long)ql[t]);
      const i32x4 D = __builtin_amdgcn_mfma_i32_16x16x32_i8(X, W, i32x4{0, 0, 0, 0}, 0, 0, 0);
      const float dw = h2f(s.dw[t]);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float dx = h2f((unsigned short)(s.dx[r] >> (16 * t)));
        acc[r] = __builtin_fmaf((float)D[r] * dw, dx, acc[r]);
      }
    }
  };
  if (u_lo < u_hi) {
    fetch(stg[0], u_lo);
    fetch(stg[1], u_lo + 1 < u_hi ? u_lo + 1 : u_hi - 1);
    for (int u = u_lo; u < u_hi; u += 2) {
      multiply(stg[0], u);
      fetch(stg[0], u + 2 < u_hi ? u + 2 : u_hi - 1);
      if (u + 1 < u_hi) multiply(stg[1], u + 1);
      fetch(stg[1], u + 3 < u_hi ? u + 3 : u_hi - 1);
    }
  }
  // the waves' tiles, summed in wave order (a wave without blocks adds zeros)
#pragma unroll
  for (int r = 0; r < 4; r++) red[(wave * 4 + r) * 64 + lane] = acc[r];
  __syncthreads();
  if (tid < 256) {
    const int r = tid >> 6;
    float sum = red[r * 64 + lane];
    for (int w = 1; w < nw; w++) sum += red[(w * 4 + r) * 64 + lane];
    const int row = r0 + x, col = 4 * g + r;
    if (row < m && col < b) out[(size_t)col * m + row] = sum;
  }
}

// ---- Q4_K / Q6_K weights x Q8_K rows -------------------------------------------------------------------------------------------
// The same split -- a workgroup per 16-row tile, its 4 or 8 waves cut the row's super-blocks between them, tiles summed in wave order,
// activation rows as operand A -- with a super-block as the unit.  Both formats keep their quants in 32-byte chunks whose low and
// high nibbles are two 32-element groups (Q4_K: the class-major pair p, sub-blocks 2p / 2p + 1; Q6_K: ql bytes 64 h + 32 (c & 1),
// units c and c + 2), and an MFMA wants 8 of a chunk's 32 bytes per lane group.  Lane (x, g) loads the 16 bytes at 16 (g & 1) of chunk
// 2 cp + (g >> 1); one v_permlane32_swap per dword pair then leaves every lane group with bytes koff(g) = 16 (g & 1) + 8 (g >> 1) ..
// + 8 of chunk 2 cp (dwords 0-1) and of chunk 2 cp + 1 (dwords 2-3).  The Q8_K row's quants (Q4_K: its class-major plane) take the same
// path, so both operands carry the same k-slot permutation.  Lane groups with g & 1 == 0 hold a chunk's first 16 elements: Q6_K's two
// 16-element scale groups are two MFMAs with the other half of the weight operand zeroed, as in k_gemm_mfma_q6k.
// Sub-block sums are folded with the 6-bit / int8 scales in integers (a lane needs the scales of ONE weight row: its own); the
// minimum term (Q4_K) and the -32 offset (Q6_K) are two more MFMAs per super-block over the row's quant sums split as 64 a + b, again
// as the int8 GEMM does.  Per super-block: acc += (d * d8) * isum - (dmin * d8) * msum (Q4_K), acc += (d * d8) * (isum - 32 osum) (Q6_K).
__device__ __forceinline__ void chunk_pair_split(i32x4 v, unsigned long long& c0, unsigned long long& c1) {
  const auto s0 = __builtin_amdgcn_permlane32_swap((unsigned)v[0], (unsigned)v[2], false, false);
  const auto s1 = __builtin_amdgcn_permlane32_swap((unsigned)v[1], (unsigned)v[3], false, false);
  c0 = ((unsigned long long)s1[0] << 32) | (unsigned long long)s0[0];
  c1 = ((unsigned long long)s1[1] << 32) | (unsigned long long)s0[1];
}
// n (4 or 8) consecutive i16 quant sums, pairs added when n == 4 words hold 8 sums -> the (b, a) bytes of sum = 64 a + b
template <int PAIRS>
__device__ __forceinline__ void split_sums(const i32x4* v, unsigned long long& lo, unsigned long long& hi) {
  lo = hi = 0ull;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    int bs;
    if constexpr (PAIRS) {
      const int w2 = v[q >> 2][q & 3];
      bs = (int)(short)(w2 & 0xffff) + (int)(short)((unsigned)w2 >> 16);
    } else {
      const int w2 = v[0][q >> 1];
      bs = (q & 1) ? (int)(short)((unsigned)w2 >> 16) : (int)(short)(w2 & 0xffff);
    }
    const int bl = ((bs + 32) & 63) - 32, bh = (bs - bl) >> 6;
    lo |= (unsigned long long)((unsigned)bl & 0xffu) << (8 * q);
    hi |= (unsigned long long)((unsigned)bh & 0xffu) << (8 * q);
  }
}

struct SkinnyGeoK {
  static constexpr int MAX_WAVES = 8;
};

template <int FMT>  // CRABML_HIP_Q4_K | CRABML_HIP_Q6_K
__global__ __launch_bounds__(512) void k_gemm_skinny_k(const char* __restrict__ w, size_t off_scale, const char* __restrict__ act,
                                                       size_t act_stride, size_t off_d, size_t off_aux, size_t off_p,
                                                       float* __restrict__ out, int m, int nsb, int b) {
  constexpr bool Q4 = FMT == CRABML_HIP_Q4_K;
  __shared__ float red[SkinnyGeoK::MAX_WAVES * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6;
  const int x = lane & 15, g = lane >> 4;
  const int r0 = (int)blockIdx.x * SkinnyGeo::ROWS;
  const int wrow = r0 + x < m ? r0 + x : m - 1;
  const int acol = x < b ? x : b - 1;
  const size_t blk0 = (size_t)wrow * nsb;
  const size_t nblk = off_scale / 128;                 // blocks in the tensor (both formats: 128 bytes of low quants per block)
  const int loff = 32 * (g >> 1) + 16 * (g & 1);       // this lane's 16 bytes inside a pair of chunks
  const char* wq = w + blk0 * 128 + loff;              // Q4_K qs / Q6_K ql
  const char* wx = w + off_scale + (Q4 ? blk0 * 16 : nblk * 64 + blk0 * 16);  // Q4_K header / Q6_K scales: 16 bytes per block
  const char* wqh = w + off_scale + blk0 * 64 + loff;  // Q6_K qh
  const unsigned short* wd = (const unsigned short*)(w + off_scale + nblk * 80) + blk0;  // Q6_K d
  const char* arow = act + (size_t)acol * act_stride;
  const char* aq = arow + (Q4 ? off_p : 0) + loff;
  const char* ab = arow + off_aux + (Q4 ? 0 : 16 * (g & 1));
  const float* adp[4];
#pragma unroll
  for (int r = 0; r < 4; r++) adp[r] = (const float*)(act + (size_t)(4 * g + r < b ? 4 * g + r : b - 1) * act_stride + off_d);

  const int per = (nsb + nw - 1) / nw;
  const int u_lo = wave * per, u_hi = u_lo + per < nsb ? u_lo + per : nsb;

  struct Stage {
    i32x4 q[2], hx, qh, xq[4], xb[Q4 ? 2 : 1];
    unsigned short d6;
    float d8[4];
  };
  Stage stg[2];
  auto fetch = [&](Stage& s, int sb) {
#pragma unroll
    for (int cp = 0; cp < 2; cp++) s.q[cp] = __builtin_nontemporal_load((const i32x4*)(wq + (size_t)sb * 128 + 64 * cp));
    s.hx = __builtin_nontemporal_load((const i32x4*)(wx + (size_t)sb * 16));
    if constexpr (!Q4) {
      s.qh = __builtin_nontemporal_load((const i32x4*)(wqh + (size_t)sb * 64));
      s.d6 = wd[sb];
    }
#pragma unroll
    for (int jj = 0; jj < 4; jj++) s.xq[jj] = *(const i32x4*)(aq + (size_t)sb * 256 + 64 * jj);
#pragma unroll
    for (int p = 0; p < (Q4 ? 2 : 1); p++) s.xb[p] = *(const i32x4*)(ab + (size_t)sb * 32 + 16 * p);
#pragma unroll
    for (int r = 0; r < 4; r++) s.d8[r] = adp[r][sb];
  };
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  auto multiply = [&](Stage& s) {
    constexpr unsigned long long NIB = 0x0F0F0F0F0F0F0F0Full;
    unsigned long long wc[4], xc[8];
#pragma unroll
    for (int cp = 0; cp < 2; cp++) chunk_pair_split(s.q[cp], wc[2 * cp], wc[2 * cp + 1]);
#pragma unroll
    for (int jj = 0; jj < 4; jj++) chunk_pair_split(s.xq[jj], xc[2 * jj], xc[2 * jj + 1]);
    int iacc[4] = {0, 0, 0, 0};
    const unsigned h0 = (unsigned)s.hx[0], h1 = (unsigned)s.hx[1], h2 = (unsigned)s.hx[2], h3 = (unsigned)s.hx[3];
    unsigned long long xl, xh, wm;
    if constexpr (Q4) {
      unsigned long long mins = 0ull;
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const unsigned f = q4k_pair_field(h1, h2, h3, p);
        mins |= (unsigned long long)(((f >> 12) & 63u) | ((f >> 18) << 8)) << (16 * p);
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const long W = (long)((e ? wc[p] >> 4 : wc[p]) & NIB);
          const i32x4 D = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)xc[2 * p + e], W, i32x4{0, 0, 0, 0}, 0, 0, 0);
          const int sc = (int)((e ? f >> 6 : f) & 63u);
#pragma unroll
          for (int r = 0; r < 4; r++) iacc[r] += __mul24(D[r], sc);
        }
      }
      split_sums<1>(s.xb, xl, xh);
      wm = g == 0 ? mins : 0ull;  // 8 minimums x 8 quant sums in k-slot group 0; the other groups feed zeros
      if (g != 0) xl = xh = 0ull;
    } else {
      unsigned long long hq[2];
      chunk_pair_split(s.qh, hq[0], hq[1]);
      const unsigned scw[4] = {h0, h1, h2, h3};
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int c = 0; c < 4; c++) {  // unit (h, c): elements 128 h + 32 c + [0, 32), scale groups 8 h + 2 c, + 1
          const unsigned long long lw = wc[2 * h + (c & 1)];
          const unsigned long long A = (((c >> 1) ? lw >> 4 : lw) & NIB) | (((hq[h] >> (2 * c)) & 0x0303030303030303ull) << 4);
          const long A0 = (g & 1) ? 0l : (long)A, A1 = (g & 1) ? (long)A : 0l;
          const long X = (long)xc[4 * h + c];
          const i32x4 D0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(X, A0, i32x4{0, 0, 0, 0}, 0, 0, 0);
          const i32x4 D1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(X, A1, i32x4{0, 0, 0, 0}, 0, 0, 0);
          const unsigned sw = scw[2 * h + (c >> 1)] >> (16 * (c & 1));
          const int s0 = (int)(signed char)(sw & 0xffu), s1 = (int)(signed char)((sw >> 8) & 0xffu);
#pragma unroll
          for (int r = 0; r < 4; r++) iacc[r] += __mul24(D0[r], s0) + __mul24(D1[r], s1);
        }
      split_sums<0>(s.xb, xl, xh);
      // 16 scales x 16 quant sums in k-slot groups 0 and 1 (group g: scales / sums 8 g .. 8 g + 7)
      wm = g == 0 ? (((unsigned long long)h1 << 32) | h0) : g == 1 ? (((unsigned long long)h3 << 32) | h2) : 0ull;
      if (g >= 2) xl = xh = 0ull;
    }
    const i32x4 Dl = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)xl, (long)wm, i32x4{0, 0, 0, 0}, 0, 0, 0);
    const i32x4 Dh = __builtin_amdgcn_mfma_i32_16x16x32_i8((long)xh, (long)wm, i32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int side = Dl[r] + 64 * Dh[r];
      if constexpr (Q4) {
        const float d = h2f((unsigned short)(h0 & 0xffffu)), dmin = h2f((unsigned short)(h0 >> 16));
        acc[r] += (d * s.d8[r]) * (float)iacc[r] - (dmin * s.d8[r]) * (float)side;
      } else {
        acc[r] += (h2f(s.d6) * s.d8[r]) * (float)(iacc[r] - 32 * side);
      }
    }
  };
  if (u_lo < u_hi) {
    fetch(stg[0], u_lo);
    fetch(stg[1], u_lo + 1 < u_hi ? u_lo + 1 : u_hi - 1);
    for (int u = u_lo; u < u_hi; u += 2) {
      multiply(stg[0]);
      fetch(stg[0], u + 2 < u_hi ? u + 2 : u_hi - 1);
      if (u + 1 < u_hi) multiply(stg[1]);
      fetch(stg[1], u + 3 < u_hi ? u + 3 : u_hi - 1);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) red[(wave * 4 + r) * 64 + lane] = acc[r];
  __syncthreads();
  if (tid < 256) {
    const int r = tid >> 6;
    float sum = red[r * 64 + lane];
    for (int wv = 1; wv < nw; wv++) sum += red[(wv * 4 + r) * 64 + lane];
    const int row = r0 + x, col = 4 * g + r;
    if (row < m && col < b) out[(size_t)col * m + row] = sum;
  }
}

// waves per row tile: 4, doubled while the grid leaves fewer than two waves per SIMD and every wave still gets two units
static int skinny_waves(const crabml_hip_device* dev, size_t row_tiles, int nunits, int max_waves) {
  int nw = 4;
  while (nw < max_waves && row_tiles * nw < (size_t)8 * dev->n_cu && 2 * nw <= nunits) nw *= 2;
  return nw;
}

// returns false when the shape / format is not covered (the caller keeps one GEMV per row).  act_qtype: the row type the planes at
// `act` were quantized to; a matrix whose format reads another one is declined, never mis-read
bool launch_gemm_skinny(crabml_hip_device* dev, const crabml_hip_buf* w, uint32_t act_qtype, size_t m, size_t k, const void* act, size_t b,
                        float* out, crabml_hip_device::ProfRec* rec) {
  const bool blocks32 = w->dtype == CRABML_HIP_Q4_0 || w->dtype == CRABML_HIP_Q8_0, kq = w->dtype == CRABML_HIP_Q4_K || w->dtype == CRABML_HIP_Q6_K;
  if ((!blocks32 && !kq) || act_qtype != vec_dot_rhs_dtype(w->dtype)) return false;
  if (b < 2 || b > 15 || m == 0 || k == 0 || k % (kq ? 256 : 32) != 0 || m > (size_t)1 << 30 || k > (size_t)1 << 30) return false;
  const ActLayout al = act_layout(act_qtype, k);
  const size_t row_tiles = (m + SkinnyGeo::ROWS - 1) / SkinnyGeo::ROWS;
  if (kq) {
    const int nsb = (int)(k / 256), nw = skinny_waves(dev, row_tiles, nsb, SkinnyGeoK::MAX_WAVES);
    with_const<CRABML_HIP_Q4_K, CRABML_HIP_Q6_K>((int)w->dtype, [&](auto f) {
      launch_k(dev->stream, rec, k_gemm_skinny_k<decltype(f)::value>, dim3((unsigned)row_tiles), dim3(64 * nw), 0, (const char*)w->ptr,
               (size_t)w->wl.off_scale, (const char*)act, al.total, al.off_d, al.off_aux, al.off_p, out, (int)m, nsb, (int)b);
    });
    return true;
  }
  const int nb = (int)(k / 32), nunits = (nb + SkinnyGeo::UNIT - 1) / SkinnyGeo::UNIT;
  const int nw = skinny_waves(dev, row_tiles, nunits, SkinnyGeo::MAX_WAVES);
  with_const<CRABML_HIP_Q4_0, CRABML_HIP_Q8_0>((int)w->dtype, [&](auto f) {
    launch_k(dev->stream, rec, k_gemm_skinny<decltype(f)::value>, dim3((unsigned)row_tiles), dim3(64 * nw), 0, (const i32x4*)w->ptr,
             scale_plane<unsigned short>(w), (const char*)act, al.total, al.off_d, out, (int)m, nb, (int)b);
  });
  return true;
}

}  // namespace crabml_hip

