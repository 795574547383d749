// gemm_mfma.hip -- matmul_vec with a batched rhs (b >= 16 rows of activations): skinny GEMM on the matrix cores.
//
// The reference runs `C[b, m] = W[m, k] . x[b, k]` as b independent dots (matmul_vec.rs:41-76); every weight row is
// streamed once per batch row.  Here one wavefront owns 16 weight rows and up to 64 batch rows and streams the
// weights ONCE: per 32-element block one `v_mfma_i32_16x16x32_i8` per 16 batch rows gives the exact integer dots
// sum_k w[i][k] x[j][k] of the 16 x 16 tile, which are then scaled exactly as the reference's scalar loop does,
// `sumf += (sumi as f32 * d_w) * d_x` (buf_q4_0.rs:249, buf_q8_0.rs:282), block after block in order -- so each
// output equals the reference's scalar-order result bit for bit (the per-block scales forbid accumulating across
// blocks inside the MFMA, which also bounds its utilisation: 4 conversions + 8 f32 ops per lane per MFMA).
//
// MFMA operand layout (16x16x32 i8): lane l supplies, for A, 8 k-slots of row i = l & 15 and, for B, the same 8
// k-slots of column j = l & 15; k-slot group = l >> 4.  The product is invariant under any permutation of the 32
// k-slots applied to both operands, so the slots are assigned for load convenience:
//   Q4_0: lane group g takes the block's quant bytes [4g, 4g+4): low nibbles = elements 4g..4g+3, high nibbles =
//         elements 16+4g..16+4g+3 (buf_q4_0.rs:24-33); the -8 offset is applied as -8 * sum(x) per block (exact);
//   Q8_0: lane group g takes elements [8g, 8g+8).
// D: lane l holds rows (l >> 4) * 4 + r (r = 0..3) of column l & 15.
#include <cstdlib>
#include <type_traits>

#include "devutil.hpp"
#include "gemv_core.hpp"
#include "kernels.hpp"

namespace crabml_hip {

// Workgroup = 4 waves = 64 weight rows x 64 batch columns; k runs in chunks of KC = 8 blocks staged through two LDS
// buffers: while a chunk is multiplied, the next one is already in flight from HBM (weights, coalesced 16-byte
// loads: one pass) and L2 (activation planes, shared by the four waves) into registers, and lands in the other
// buffer behind a single barrier per chunk.  LDS rows are [block][row or column][RW words] with RW = 4 (Q4_0
// quants) or 12 (8 data words + 4 pad): staging writes are 16-byte vectors and a wave's fragment reads (lane =
// (i, g): words g / 4 + g, or 2g / 2g + 1, of row i) hit every bank exactly twice.
template <int FMT, int NT>  // NT column tiles of 16 batch rows per workgroup (4, or 2 when the grid would not fill the chip)
struct GemmGeo {
  static constexpr int CW = 16 * NT;                               // batch rows per workgroup
  static constexpr int KC = 4;                                     // blocks per chunk (37 KB of LDS per workgroup: 4 workgroups per CU)
  static constexpr int APC = (FMT == CRABML_HIP_Q4_0 || FMT == CRABML_HIP_Q4_1) ? 1 : 2;       // 16-byte pieces per weight block
  static constexpr int ARW = (FMT == CRABML_HIP_Q4_0 || FMT == CRABML_HIP_Q4_1) ? 4 : 12;      // LDS words per weight block row
  static constexpr int BRW = 12;                                   // LDS words per activation block row
  static constexpr int A_WORDS = KC * 64 * ARW, B_WORDS = KC * CW * BRW;
  // one buffer: A quants | B quants | A scales f32 [KC][64] | B scales f32 [KC][64] (converted from f16 once, by the
  // staging threads, instead of once per wave and block)
  static constexpr int BUF_BYTES = (A_WORDS + B_WORDS) * 4 + KC * 64 * 4 * 2;
  static constexpr int LDS_BYTES = 2 * BUF_BYTES;
  static constexpr int A_LOADS = 64 * KC * APC / 256, B_LOADS = CW * KC * 2 / 256, S_LOADS = 64 * KC / 256;
};

// FMA (the fast prompt pass only, crabml_hip_llama_prefill): sumf = fma(sumi as f32 * d_w, d_x, sumf) -- the block term's second
// product and the add as one v_pk_fma_f32 (8 instead of 10 VALU operations per MFMA; one rounding fewer than the reference's
// expression, the same distance the fast decode step's re-associated sums are allowed).  matmul_vec itself and the strict-order
// device keep the reference's three roundings (bit-exact, tests/test_hip_gemv.py).
template <int FMT, int NT, bool FMA = false>
__global__ __launch_bounds__(256) void k_gemm_mfma(const char* __restrict__ wq, const unsigned short* __restrict__ wd,
                                                   const char* __restrict__ act, size_t act_stride, size_t off_d, size_t off_aux,
                                                   float* __restrict__ out, int m, int nb, int b, int row_tiles) {
  using G = GemmGeo<FMT, NT>;
  constexpr int KC = G::KC, APC = G::APC, ARW = G::ARW, BRW = G::BRW, CW = G::CW;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Tile order.  Workgroup b runs on XCD b % 8 and the eight L2s do not share: all column tiles of a weight row tile
  // must sit on ONE XCD, back to back, or every column tile re-fetches the weights (rocprofv3 FETCH_SIZE: 294 MB per
  // 35 MB gate/up GEMM with column-major tile order).  XCD x owns the row tiles rt = x (mod 8); its j-th workgroup
  // is (rt = 8 (j / col_tiles) + x, ct = j % col_tiles).  The activation tiles (8 x 295 KB) stay L2-resident.
  int rt, ct;
  {
    const int col_tiles = (int)gridDim.x / row_tiles;
    if ((row_tiles & 7) == 0) {
      const int x = (int)blockIdx.x & 7, j = (int)blockIdx.x >> 3;
      ct = j % col_tiles;
      rt = (j / col_tiles) * 8 + x;
    } else {
      rt = (int)blockIdx.x % row_tiles;
      ct = (int)blockIdx.x / row_tiles;
    }
  }
  const int r0 = rt * 64, c0 = ct * CW;
  const int i = lane & 15, g = lane >> 4;

  // staging registers: PF chunks in flight (a k-chunk's global loads are issued PF - 1 iterations before they are
  // committed to LDS: with one chunk of slack a workgroup's serial chain of nb / KC chunks ran at the HBM round trip
  // per chunk -- 4096 x 14336 took the same 134 us for 64 and for 256 batch rows)
  constexpr int PF = 2;
  struct Stage {
    i32x4 ra[G::A_LOADS], rb[G::B_LOADS];
    unsigned rad[G::S_LOADS], rbd[G::S_LOADS];  // f16 scale bits; Q4_1: (d | m << 16) and the Q8_1 row's (d | s << 16)
  };
  Stage stg[PF];
  auto fetch = [&](auto SET, int kb0) {
    auto& ra = stg[decltype(SET)::value].ra;
    auto& rb = stg[decltype(SET)::value].rb;
    auto& rad = stg[decltype(SET)::value].rad;
    auto& rbd = stg[decltype(SET)::value].rbd;
#pragma unroll
    for (int u = 0; u < G::A_LOADS; u++) {
      const int t = tid + 256 * u, row = t / (KC * APC), rem = t % (KC * APC), kb = rem / APC, pc = rem % APC;
      const int grow = r0 + row < m ? r0 + row : m - 1;
      const int gkb = kb0 + kb < nb ? kb0 + kb : nb - 1;  // the tail chunk re-reads the last block (never consumed)
      ra[u] = __builtin_nontemporal_load((const i32x4*)wq + ((size_t)grow * nb + gkb) * APC + pc);
    }
#pragma unroll
    for (int u = 0; u < G::B_LOADS; u++) {
      const int t = tid + 256 * u, col = t / (KC * 2), rem = t % (KC * 2), kb = rem / 2, pc = rem % 2;
      const int gcol = c0 + col < b ? c0 + col : b - 1;
      const int gkb = kb0 + kb < nb ? kb0 + kb : nb - 1;
      rb[u] = *((const i32x4*)(act + (size_t)gcol * act_stride) + (size_t)gkb * 2 + pc);
    }
#pragma unroll
    for (int u = 0; u < G::S_LOADS; u++) {
      const int t = tid + 256 * u, rc = t / KC, kb = t % KC;
      const int grow = r0 + rc < m ? r0 + rc : m - 1, gcol = c0 + rc < b ? c0 + rc : b - 1;
      const int gkb = kb0 + kb < nb ? kb0 + kb : nb - 1;
      const char* ap = act + (size_t)gcol * act_stride;
      if constexpr (FMT == CRABML_HIP_Q4_1) {
        rad[u] = ((const unsigned*)wd)[(size_t)grow * nb + gkb];
        rbd[u] = (unsigned)((const unsigned short*)(ap + off_d))[gkb] | ((unsigned)((const unsigned short*)(ap + off_aux))[gkb] << 16);
      } else {
        rad[u] = wd[(size_t)grow * nb + gkb];
        rbd[u] = ((const unsigned short*)(ap + off_d))[gkb];
      }
    }
  };
  auto commit = [&](auto SET, int buf) {
    auto& ra = stg[decltype(SET)::value].ra;
    auto& rb = stg[decltype(SET)::value].rb;
    auto& rad = stg[decltype(SET)::value].rad;
    auto& rbd = stg[decltype(SET)::value].rbd;
    unsigned* sA = (unsigned*)(lds_raw + (size_t)buf * G::BUF_BYTES);
    unsigned* sB = sA + G::A_WORDS;
    float* sAd = (float*)(sB + G::B_WORDS);
    float* sBd = sAd + KC * 64;
#pragma unroll
    for (int u = 0; u < G::A_LOADS; u++) {
      const int t = tid + 256 * u, row = t / (KC * APC), rem = t % (KC * APC), kb = rem / APC, pc = rem % APC;
      *(i32x4*)(sA + (kb * 64 + row) * ARW + pc * 4) = ra[u];
    }
#pragma unroll
    for (int u = 0; u < G::B_LOADS; u++) {
      const int t = tid + 256 * u, col = t / (KC * 2), rem = t % (KC * 2), kb = rem / 2, pc = rem % 2;
      if constexpr (FMT == CRABML_HIP_Q4_0) {
        // lane group g multiplies the block's elements [4 g, 4 g + 4) and [16 + 4 g, ..): dword g of piece 0 and of piece 1 go side
        // by side, so that the fragment is ONE 8-byte LDS read (the LDS pipe is what this kernel saturates: every instruction
        // costs it ~8 cycles whatever its width -- rocprofv3 SQ_ACTIVE_INST_LDS / SQ_INSTS_LDS, profiles/r05_prefill_gemm_experiments.md)
        unsigned* brow = sB + (kb * CW + col) * BRW + pc;
        brow[0] = (unsigned)rb[u][0];
        brow[2] = (unsigned)rb[u][1];
        brow[4] = (unsigned)rb[u][2];
        brow[6] = (unsigned)rb[u][3];
      } else {
        *(i32x4*)(sB + (kb * CW + col) * BRW + pc * 4) = rb[u];
      }
    }
#pragma unroll
    for (int u = 0; u < G::S_LOADS; u++) {
      const int t = tid + 256 * u, rc = t / KC, kb = t % KC;
      if constexpr (FMT == CRABML_HIP_Q4_1) {  // raw f16 pairs: the products are taken in f16 (buf_q4_1.rs:276)
        ((unsigned*)sAd)[kb * 64 + rc] = rad[u];
        ((unsigned*)sBd)[kb * 64 + rc] = rbd[u];
      } else {
        sAd[kb * 64 + rc] = h2f((unsigned short)rad[u]);
        // (the activation scales of a lane's NT column tiles side by side: one 16-byte read per block instead of NT reads)
        sBd[kb * 64 + (rc & 15) * 4 + (rc >> 4)] = h2f((unsigned short)rbd[u]);
      }
    }
  };

  // accumulators as f32 pairs: the block scaling runs on v_pk_mul_f32 / v_pk_add_f32 (same IEEE operations, two
  // rows per instruction)
  f32x2 F[NT][2];
  float Fq[NT][4];  // Q4_1 only: scalar accumulators (element-wise updates of the ext-vector ones were miscompiled)
#pragma unroll
  for (int jt = 0; jt < NT; jt++) {
    F[jt][0] = F[jt][1] = f32x2{0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; r++) Fq[jt][r] = 0.0f;
  }

  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>;
  const int nchunks = (nb + KC - 1) / KC;
  // every fetch / commit below is unconditional (chunk indices past the end are clamped: they re-read the last
  // chunk and are never multiplied): with a fixed number of loads per iteration the compiler's s_waitcnt vmcnt(n)
  // before a commit waits for exactly the loads of that chunk; with conditional fetches it fell back to waiting
  // for everything in flight, i.e. one HBM round trip per chunk
  const int last = (nchunks - 1) * KC;
  fetch(S0{}, 0);
  commit(S0{}, 0);
  fetch(S1{}, KC < last ? KC : last);
  if constexpr (PF == 3) fetch(S2{}, 2 * KC < last ? 2 * KC : last);
  __syncthreads();
  // per-lane LDS offsets (words), constant over the k loop: the block index only adds immediates
  const int a_off = (16 * wave + i) * ARW + ((FMT == CRABML_HIP_Q4_0 || FMT == CRABML_HIP_Q4_1) ? g : 2 * g);
  const int ad_off = 16 * wave + 4 * g;
  // iteration c: request chunk c + PF into the set chunk c used, multiply chunk c (LDS buffer c & 1), commit chunk
  // c + 1 (requested two iterations ago) to the other buffer, barrier
  auto step = [&](auto SET_C, auto SET_N, int c) {
    const int kb0 = c * KC, buf = c & 1;
    const int kc = c >= nchunks ? 0 : nb - kb0 < KC ? nb - kb0 : KC;
    fetch(SET_C, (c + PF) * KC < last ? (c + PF) * KC : last);
    const unsigned* sA = (const unsigned*)(lds_raw + (size_t)buf * G::BUF_BYTES);
    const unsigned* sB = sA + G::A_WORDS;
    const float* sAd = (const float*)(sB + G::B_WORDS);
    const float* sBd = sAd + KC * 64;
    auto mul_block = [&](int kb) {
      if constexpr (FMT == CRABML_HIP_Q4_1) {
        // Q4_1 x Q8_1 (buf_q4_1.rs:270-280): unsigned nibbles, per block sumf += f16(d_w * d_x) * sumi + f16(m_w * s_x)
        // with both products rounded to f16 -- in block order, i.e. the scalar reference bit for bit
        const unsigned w = sA[kb * 64 * ARW + a_off];
        const long A1 = (long)(((unsigned long long)((w >> 4) & 0x0F0F0F0Fu) << 32) | (unsigned long long)(w & 0x0F0F0F0Fu));
        const i32x4 dm4 = *(const i32x4*)((const unsigned*)sAd + kb * 64 + ad_off);
        unsigned dmr[4] = {(unsigned)dm4[0], (unsigned)dm4[1], (unsigned)dm4[2], (unsigned)dm4[3]};
#pragma unroll
        for (int jt = 0; jt < NT; jt++) {
          const int col = 16 * jt + i;
          const unsigned* brow = sB + (kb * CW + col) * BRW;
          const long Bf1 = (long)(((unsigned long long)brow[4 + g] << 32) | (unsigned long long)brow[g]);
          const unsigned ds = ((const unsigned*)sBd)[kb * 64 + col];
          const i32x4 D1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(A1, Bf1, i32x4{0, 0, 0, 0}, 0, 0, 0);
          const unsigned short dxh = (unsigned short)(ds & 0xffffu), sxh = (unsigned short)(ds >> 16);
          const int Dr[4] = {D1[0], D1[1], D1[2], D1[3]};
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float a = h2f(h_mul((unsigned short)(dmr[r] & 0xffffu), dxh));
            const float bm = h2f(h_mul((unsigned short)(dmr[r] >> 16), sxh));
            Fq[jt][r] += a * (float)Dr[r] + bm;
          }
        }
        return;
      }
      long A;
      if (FMT == CRABML_HIP_Q4_0) {
        // nibbles to signed bytes v - 8 without carries between bytes: ((v | 0x80) - 8) ^ 0x80 per byte, so the
        // MFMA accumulates the reference's (q - 8) * x directly (buf_q4_0.rs:245-248) and starts from zero
        const unsigned w = sA[kb * 64 * ARW + a_off];
        const unsigned lo = (((w & 0x0F0F0F0Fu) | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
        const unsigned hi = ((((w >> 4) & 0x0F0F0F0Fu) | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
        A = (long)(((unsigned long long)hi << 32) | (unsigned long long)lo);
      } else {
        A = *(const long*)(sA + kb * 64 * ARW + a_off);
      }
      const f32x4 dw4 = *(const f32x4*)(sAd + kb * 64 + ad_off);
      const f32x2 dw01 = {dw4[0], dw4[1]}, dw23 = {dw4[2], dw4[3]};
      // all four column tiles: fragments first, then the four MFMAs back to back (independent accumulators),
      // then the scaling
      long Bf[NT];
      float dx[NT];
#pragma unroll
      for (int jt = 0; jt < NT; jt++) {
        const int col = 16 * jt + i;
        const unsigned* brow = sB + (kb * CW + col) * BRW;
        if (FMT == CRABML_HIP_Q4_0)
          Bf[jt] = *(const long*)(brow + 2 * g);  // (dword g of piece 0 | dword g of piece 1: see commit)
        else
          Bf[jt] = *(const long*)(brow + 2 * g);
      }
      {
        const f32x4 dx4 = *(const f32x4*)(sBd + kb * 64 + i * 4);
#pragma unroll
        for (int jt = 0; jt < NT; jt++) dx[jt] = dx4[jt];
      }
      i32x4 D[NT];
#pragma unroll
      for (int jt = 0; jt < NT; jt++) D[jt] = __builtin_amdgcn_mfma_i32_16x16x32_i8(A, Bf[jt], i32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
      for (int jt = 0; jt < NT; jt++) {
        const f32x2 c01 = {(float)D[jt][0], (float)D[jt][1]}, c23 = {(float)D[jt][2], (float)D[jt][3]};
        const f32x2 dxx = {dx[jt], dx[jt]};
        if constexpr (FMA) {
          F[jt][0] = __builtin_elementwise_fma(c01 * dw01, dxx, F[jt][0]);
          F[jt][1] = __builtin_elementwise_fma(c23 * dw23, dxx, F[jt][1]);
        } else {
          F[jt][0] += (c01 * dw01) * dxx;  // sumf += (sumi as f32 * d_w) * d_x, block after block
          F[jt][1] += (c23 * dw23) * dxx;
        }
      }
    };
    if (kc == KC) {  // straight-line: the scheduler may start block kb + 1's LDS reads under block kb's scaling
#pragma unroll
      for (int kb = 0; kb < KC; kb++) mul_block(kb);
    } else {  // ragged k, or an iteration past the end (kc = 0)
      for (int kb = 0; kb < kc; kb++) mul_block(kb);
    }
    commit(SET_N, buf ^ 1);  // that buffer was last read one iteration ago (barrier below)
    __syncthreads();
  };
  for (int c = 0; c < nchunks; c += PF) {
    if constexpr (PF == 3) {
      step(S0{}, S1{}, c);
      step(S1{}, S2{}, c + 1);
      step(S2{}, S0{}, c + 2);
    } else {
      step(S0{}, S1{}, c);
      step(S1{}, S0{}, c + 1);
    }
  }
#pragma unroll
  for (int jt = 0; jt < NT; jt++) {
    const int col = c0 + 16 * jt + i;
    if (col >= b) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = r0 + 16 * wave + g * 4 + r;
      if (row < m) out[(size_t)col * m + row] = FMT == CRABML_HIP_Q4_1 ? Fq[jt][r] : F[jt][r >> 1][r & 1];
    }
  }
}

// ---- Q4_K weights x Q8_K activation rows (the prompt of a *_K_M file) ------------------------------------------------
// One chunk = one 256-element super-block.  Per 32-element sub-block j one MFMA per 16 x 16 tile gives the exact integer
// dots sum q4 * q8 (nibbles are unsigned: Q4_K has no -8 offset), which are folded into the super-block sum with the
// sub-block's 6-bit scale IN INTEGERS (v_mad_i32_i24; |sum| < 2^24) -- no conversion and no float work per sub-block,
// which is what bounds the Q4_0 kernel.  The minimum term sum_j m_j * bsum_j is two more MFMAs per tile and
// super-block: operand A = the row's eight 6-bit minimums, operand B = the column's eight 32-element quant sums split as
// bsum = 64 a + b with b in [-32, 32), a in [-64, 64] (both fit int8).  Per super-block and output then, as the GEMV
// does (buf_q4_k.rs:200-262): acc += (d * d8) * isum - (dmin * d8) * msum.
// Operand layout as above: lane (i, g) supplies bytes [8g, 8g + 8) of the sub-block for row / column i; low nibbles of
// qs bytes [32p, 32p + 32) are sub-block 2p, high nibbles sub-block 2p + 1 (buf_q4_k.rs:212-217).
template <int NT>
struct GemmGeoK {
  static constexpr int CW = 16 * NT;
  static constexpr int ASTR = 36;  // words per weight row: 128 B of quants + 16 B pad (16-byte aligned rows)
  static constexpr int BSTR = 68;  // words per activation row: 256 B + 16 B pad
  // one buffer, in words: A quants | A scales (8 bytes / row) | A mins | A d f32 | A dmin f32 | B quants | B d8 f32 |
  // B bsum low parts (8 bytes / column) | B bsum high parts
  static constexpr int O_ASC = 64 * ASTR, O_AM = O_ASC + 128, O_AD = O_AM + 128, O_ADM = O_AD + 64, O_BQ = O_ADM + 64;
  static constexpr int O_BD = O_BQ + CW * BSTR, O_BLO = O_BD + CW, O_BHI = O_BLO + 2 * CW, BUF_WORDS = O_BHI + 2 * CW;
  static constexpr int LDS_BYTES = 2 * BUF_WORDS * 4;
  static constexpr int A_LOADS = 2, B_LOADS = CW * 16 / 256;
};

template <int NT>
__global__ __launch_bounds__(256) void k_gemm_mfma_q4k(const i32x4* __restrict__ wq, const i32x4* __restrict__ wh,
                                                       const char* __restrict__ act, size_t act_stride, size_t off_d, size_t off_aux,
                                                       size_t off_p, float* __restrict__ out, int m, int nsb, int b, int row_tiles,
                                                       int* __restrict__ dbg) {
  using G = GemmGeoK<NT>;
  constexpr int CW = G::CW;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  int rt, ct;
  {  // XCD-aware tile order (see k_gemm_mfma)
    const int col_tiles = (int)gridDim.x / row_tiles;
    if ((row_tiles & 7) == 0) {
      const int x = (int)blockIdx.x & 7, j = (int)blockIdx.x >> 3;
      ct = j % col_tiles;
      rt = (j / col_tiles) * 8 + x;
    } else {
      rt = (int)blockIdx.x % row_tiles;
      ct = (int)blockIdx.x / row_tiles;
    }
  }
  const int r0 = rt * 64, c0 = ct * CW;

  i32x4 ra[G::A_LOADS], rb[G::B_LOADS], rh, rbs;
  float rd8 = 0.f;
  auto fetch = [&](int sb) {
#pragma unroll
    for (int u = 0; u < G::A_LOADS; u++) {
      const int t = tid + 256 * u, row = t >> 3, pc = t & 7;
      const int grow = r0 + row < m ? r0 + row : m - 1;
      ra[u] = __builtin_nontemporal_load(wq + ((size_t)grow * nsb + sb) * 8 + pc);
    }
    if (tid < 64) {
      const int grow = r0 + tid < m ? r0 + tid : m - 1;
      rh = __builtin_nontemporal_load(wh + (size_t)grow * nsb + sb);
    }
#pragma unroll
    for (int u = 0; u < G::B_LOADS; u++) {
      const int t = tid + 256 * u, col = t >> 4, pc = t & 15;
      const int gcol = c0 + col < b ? c0 + col : b - 1;
      rb[u] = *((const i32x4*)(act + (size_t)gcol * act_stride + off_p) + (size_t)sb * 16 + pc);  // the class-major plane (common.hpp)
    }
    if (tid < CW) {
      const int gcol = c0 + tid < b ? c0 + tid : b - 1;
      rd8 = ((const float*)(act + (size_t)gcol * act_stride + off_d))[sb];
    }
    if (tid < 2 * CW) {
      const int col = tid >> 1, gcol = c0 + col < b ? c0 + col : b - 1;
      rbs = *((const i32x4*)(act + (size_t)gcol * act_stride + off_aux) + (size_t)sb * 2 + (tid & 1));  // 8 of the 16 bsums
    }
  };
  auto commit = [&](int buf) {
    unsigned* S = (unsigned*)lds_raw + (size_t)buf * G::BUF_WORDS;
#pragma unroll
    for (int u = 0; u < G::A_LOADS; u++) {
      const int t = tid + 256 * u, row = t >> 3, pc = t & 7;
      *(i32x4*)(S + row * G::ASTR + pc * 4) = ra[u];
    }
    if (tid < 64) {  // unpack the row's header once: 8 scales, 8 mins (6 bits each), d, dmin
      const unsigned h0 = (unsigned)rh[0], h1 = (unsigned)rh[1], h2 = (unsigned)rh[2], h3 = (unsigned)rh[3];
      unsigned sc[2] = {0u, 0u}, mn[2] = {0u, 0u};
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const unsigned f = q4k_pair_field(h1, h2, h3, p);
        const unsigned s2 = (f & 63u) | (((f >> 6) & 63u) << 8), m2 = ((f >> 12) & 63u) | ((f >> 18) << 8);
        sc[p >> 1] |= s2 << (16 * (p & 1));
        mn[p >> 1] |= m2 << (16 * (p & 1));
      }
      S[G::O_ASC + tid * 2] = sc[0];
      S[G::O_ASC + tid * 2 + 1] = sc[1];
      S[G::O_AM + tid * 2] = mn[0];
      S[G::O_AM + tid * 2 + 1] = mn[1];
      ((float*)S)[G::O_AD + tid] = h2f((unsigned short)(h0 & 0xffffu));
      ((float*)S)[G::O_ADM + tid] = h2f((unsigned short)(h0 >> 16));
    }
#pragma unroll
    for (int u = 0; u < G::B_LOADS; u++) {
      const int t = tid + 256 * u, col = t >> 4, pc = t & 15;
      *(i32x4*)(S + G::O_BQ + col * G::BSTR + pc * 4) = rb[u];
    }
    if (tid < CW) ((float*)S)[G::O_BD + tid] = rd8;
    if (tid < 2 * CW) {  // four 32-element quant sums -> (b, a) byte pairs: bsum = 64 a + b
      unsigned lo = 0u, hi = 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int w2 = rbs[q];
        const int bs = (int)(short)(w2 & 0xffff) + (int)(short)((unsigned)w2 >> 16);
        const int bl = ((bs + 32) & 63) - 32, bh = (bs - bl) >> 6;
        lo |= ((unsigned)bl & 0xffu) << (8 * q);
        hi |= ((unsigned)bh & 0xffu) << (8 * q);
      }
      S[G::O_BLO + tid] = lo;  // column tid / 2, half tid & 1: words [2 col + half]
      S[G::O_BHI + tid] = hi;
    }
  };

  f32x2 F[NT][2];
#pragma unroll
  for (int jt = 0; jt < NT; jt++) F[jt][0] = F[jt][1] = f32x2{0.0f, 0.0f};

  fetch(0);
  commit(0);
  __syncthreads();
  for (int sb = 0; sb < nsb; sb++) {
    const int buf = sb & 1;
    fetch(sb + 1 < nsb ? sb + 1 : sb);  // unconditional (the last one re-reads): in flight while this chunk is multiplied
    const unsigned* S = (const unsigned*)lds_raw + (size_t)buf * G::BUF_WORDS;
    const unsigned* arow = S + (16 * wave + i) * G::ASTR + 2 * g;
    // scales / d / dmin of the four rows this lane's accumulators belong to (rows 4g .. 4g + 3 of the wave's 16)
    unsigned long long sc8[4];
#pragma unroll
    for (int r = 0; r < 4; r++) sc8[r] = *(const unsigned long long*)(S + G::O_ASC + (16 * wave + 4 * g + r) * 2);
    const f32x4 dw4 = *(const f32x4*)((const float*)S + G::O_AD + 16 * wave + 4 * g);
    const f32x4 dm4 = *(const f32x4*)((const float*)S + G::O_ADM + 16 * wave + 4 * g);
    int iacc[NT][4];
#pragma unroll
    for (int jt = 0; jt < NT; jt++)
#pragma unroll
      for (int r = 0; r < 4; r++) iacc[jt][r] = 0;
#pragma unroll 2
    for (int j = 0; j < 8; j++) {  // (fully unrolled the compiler hoists every fragment read: 268 VGPRs)
      const unsigned long long aw = *(const unsigned long long*)(arow + 8 * (j >> 1));
      const long A = (long)(((j & 1) ? (aw >> 4) : aw) & 0x0F0F0F0F0F0F0F0Full);
      i32x4 D[NT];
#pragma unroll
      for (int jt = 0; jt < NT; jt++) {
        const long Bf = *(const long*)(S + G::O_BQ + (16 * jt + i) * G::BSTR + 8 * j + 2 * g);
        D[jt] = __builtin_amdgcn_mfma_i32_16x16x32_i8(A, Bf, i32x4{0, 0, 0, 0}, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int scj = (int)((sc8[r] >> (8 * j)) & 0xffull);
#pragma unroll
        for (int jt = 0; jt < NT; jt++) iacc[jt][r] += __mul24(D[jt][r], scj);  // v_mad_i32_i24: |D| < 2^17, scj < 64
      }
    }
    // minimum term: (8 mins of row i) x (8 quant-sum parts of column i), in k-slot group 0; the other groups feed zeros
    const long Am = g == 0 ? *(const long*)(S + G::O_AM + (16 * wave + i) * 2) : 0l;
    const f32x2 dw01 = {dw4[0], dw4[1]}, dw23 = {dw4[2], dw4[3]}, dm01 = {dm4[0], dm4[1]}, dm23 = {dm4[2], dm4[3]};
#pragma unroll
    for (int jt = 0; jt < NT; jt++) {
      const long Bl = g == 0 ? *(const long*)(S + G::O_BLO + (16 * jt + i) * 2) : 0l;
      const long Bh = g == 0 ? *(const long*)(S + G::O_BHI + (16 * jt + i) * 2) : 0l;
      const i32x4 Dl = __builtin_amdgcn_mfma_i32_16x16x32_i8(Am, Bl, i32x4{0, 0, 0, 0}, 0, 0, 0);
      const i32x4 Dh = __builtin_amdgcn_mfma_i32_16x16x32_i8(Am, Bh, i32x4{0, 0, 0, 0}, 0, 0, 0);
      const float d8 = ((const float*)S)[G::O_BD + 16 * jt + i];
      const f32x2 d88 = {d8, d8};
      const f32x2 i01 = {(float)iacc[jt][0], (float)iacc[jt][1]}, i23 = {(float)iacc[jt][2], (float)iacc[jt][3]};
      const f32x2 m01 = {(float)(Dl[0] + 64 * Dh[0]), (float)(Dl[1] + 64 * Dh[1])};
      const f32x2 m23 = {(float)(Dl[2] + 64 * Dh[2]), (float)(Dl[3] + 64 * Dh[3])};
      if (dbg != nullptr) {  // parity hook (crabml_hip_debug_gemm_ints; NULL in every product launch): this super-block's
        const int col = c0 + 16 * jt + i;  // (isum, msum) per output, exactly as the float part below consumes them
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = r0 + 16 * wave + g * 4 + r;
          if (col < b && row < m) {
            int* o = dbg + (((size_t)col * m + row) * nsb + sb) * 2;
            o[0] = iacc[jt][r];
            o[1] = Dl[r] + 64 * Dh[r];
          }
        }
      }
      F[jt][0] += (dw01 * d88) * i01 - (dm01 * d88) * m01;
      F[jt][1] += (dw23 * d88) * i23 - (dm23 * d88) * m23;
    }
    commit(buf ^ 1);  // the other buffer was last read one iteration ago (barrier below)
    __syncthreads();
  }
#pragma unroll
  for (int jt = 0; jt < NT; jt++) {
    const int col = c0 + 16 * jt + i;
    if (col >= b) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = r0 + 16 * wave + g * 4 + r;
      if (row < m) out[(size_t)col * m + row] = F[jt][r >> 1][r & 1];
    }
  }
}

// ---- Q6_K weights x Q8_K activation rows (attn_v / ffn_down / the classifier of the *_K_M mixes) -------------------------
// A Q6_K scale covers 16 elements, an MFMA 32: every 32-element unit (h, c) = elements 128 h + 32 c + [0, 32) of the
// super-block is multiplied twice with half of operand A zeroed (k-slot groups 0-1 = the unit's first scale group,
// 2-3 = the second), giving the two exact integer dots sum q6 * q8 -- the matrix cores have the headroom, the VALU is what
// is scarce.  6-bit values are rebuilt as bytes from ql (nibble c >> 1 of byte 64 h + 32 (c & 1) + l) and qh (bits 2c,
// 2c + 1 of byte 32 h + l) (buf_q6_k.rs:21-48).  Folded in integers with the int8 group scales; the -32 offset is
// -32 * sum_g scale_g * bsum_g, one more pair of MFMAs per tile and super-block (bsum = 64 a + b as for Q4_K).
// Per super-block and output: acc += (d * d8) * (sum_g scale_g * dot_g - 32 * sum_g scale_g * bsum_g).
struct GemmGeo6 {
  static constexpr int NT = 2, CW = 32;
  static constexpr int QLSTR = 36, QHSTR = 20, BSTR = 68;
  // words: A ql | A qh | A scales (16 bytes / row) | A d f32 | B quants | B d8 f32 | B bsum low parts (16 bytes / column) | high
  static constexpr int O_QH = 64 * QLSTR, O_SC = O_QH + 64 * QHSTR, O_D = O_SC + 64 * 4, O_BQ = O_D + 64;
  static constexpr int O_BD = O_BQ + CW * BSTR, O_BLO = O_BD + CW, O_BHI = O_BLO + 4 * CW, BUF_WORDS = O_BHI + 4 * CW;
  static constexpr int LDS_BYTES = 2 * BUF_WORDS * 4;
};

__global__ __launch_bounds__(256) void k_gemm_mfma_q6k(const char* __restrict__ w, size_t off_qh, const char* __restrict__ act,
                                                       size_t act_stride, size_t off_d, size_t off_aux, float* __restrict__ out,
                                                       int m, int nsb, int b, int row_tiles, int* __restrict__ dbg) {
  using G = GemmGeo6;
  constexpr int NT = G::NT, CW = G::CW;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  int rt, ct;
  {
    const int col_tiles = (int)gridDim.x / row_tiles;
    if ((row_tiles & 7) == 0) {
      const int x = (int)blockIdx.x & 7, j = (int)blockIdx.x >> 3;
      ct = j % col_tiles;
      rt = (j / col_tiles) * 8 + x;
    } else {
      rt = (int)blockIdx.x % row_tiles;
      ct = (int)blockIdx.x / row_tiles;
    }
  }
  const int r0 = rt * 64, c0 = ct * CW;
  const size_t nblk = off_qh / 128;  // blocks in the tensor
  const i32x4* wql = (const i32x4*)w;
  const i32x4* wqh = (const i32x4*)(w + off_qh);
  const i32x4* wsc = (const i32x4*)(w + off_qh + nblk * 64);
  const unsigned short* wd = (const unsigned short*)(w + off_qh + nblk * 80);

  i32x4 rql[2], rqh, rsc, rb[2], rbs;
  unsigned short rdw = 0;
  float rd8 = 0.f;
  auto fetch = [&](int sb) {
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int t = tid + 256 * u, row = t >> 3, pc = t & 7;
      const int grow = r0 + row < m ? r0 + row : m - 1;
      rql[u] = __builtin_nontemporal_load(wql + ((size_t)grow * nsb + sb) * 8 + pc);
    }
    {
      const int row = tid >> 2, pc = tid & 3;
      const int grow = r0 + row < m ? r0 + row : m - 1;
      rqh = __builtin_nontemporal_load(wqh + ((size_t)grow * nsb + sb) * 4 + pc);
    }
    if (tid < 64) {
      const int grow = r0 + tid < m ? r0 + tid : m - 1;
      rsc = __builtin_nontemporal_load(wsc + (size_t)grow * nsb + sb);
      rdw = wd[(size_t)grow * nsb + sb];
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int t = tid + 256 * u, col = t >> 4, pc = t & 15;
      const int gcol = c0 + col < b ? c0 + col : b - 1;
      rb[u] = *((const i32x4*)(act + (size_t)gcol * act_stride) + (size_t)sb * 16 + pc);
    }
    if (tid < CW) {
      const int gcol = c0 + tid < b ? c0 + tid : b - 1;
      rd8 = ((const float*)(act + (size_t)gcol * act_stride + off_d))[sb];
    }
    if (tid < 2 * CW) {
      const int col = tid >> 1, gcol = c0 + col < b ? c0 + col : b - 1;
      rbs = *((const i32x4*)(act + (size_t)gcol * act_stride + off_aux) + (size_t)sb * 2 + (tid & 1));  // 8 of the 16 bsums
    }
  };
  auto commit = [&](int buf) {
    unsigned* S = (unsigned*)lds_raw + (size_t)buf * G::BUF_WORDS;
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int t = tid + 256 * u, row = t >> 3, pc = t & 7;
      *(i32x4*)(S + row * G::QLSTR + pc * 4) = rql[u];
    }
    *(i32x4*)(S + G::O_QH + (tid >> 2) * G::QHSTR + (tid & 3) * 4) = rqh;
    if (tid < 64) {
      *(i32x4*)(S + G::O_SC + tid * 4) = rsc;
      ((float*)S)[G::O_D + tid] = h2f(rdw);
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int t = tid + 256 * u, col = t >> 4, pc = t & 15;
      *(i32x4*)(S + G::O_BQ + col * G::BSTR + pc * 4) = rb[u];
    }
    if (tid < CW) ((float*)S)[G::O_BD + tid] = rd8;
    if (tid < 2 * CW) {  // eight 16-element quant sums -> (b, a) byte pairs: bsum = 64 a + b
      unsigned lo[2] = {0u, 0u}, hi[2] = {0u, 0u};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int w2 = rbs[q];
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int bs = e ? (int)(short)((unsigned)w2 >> 16) : (int)(short)(w2 & 0xffff);
          const int bl = ((bs + 32) & 63) - 32, bh = (bs - bl) >> 6;
          const int k = 2 * q + e;  // 0..7 within this half
          lo[k >> 2] |= ((unsigned)bl & 0xffu) << (8 * (k & 3));
          hi[k >> 2] |= ((unsigned)bh & 0xffu) << (8 * (k & 3));
        }
      }
      const int col = tid >> 1, half = tid & 1;
      S[G::O_BLO + col * 4 + half * 2] = lo[0];
      S[G::O_BLO + col * 4 + half * 2 + 1] = lo[1];
      S[G::O_BHI + col * 4 + half * 2] = hi[0];
      S[G::O_BHI + col * 4 + half * 2 + 1] = hi[1];
    }
  };

  f32x2 F[NT][2];
#pragma unroll
  for (int jt = 0; jt < NT; jt++) F[jt][0] = F[jt][1] = f32x2{0.0f, 0.0f};

  fetch(0);
  commit(0);
  __syncthreads();
  for (int sb = 0; sb < nsb; sb++) {
    const int buf = sb & 1;
    fetch(sb + 1 < nsb ? sb + 1 : sb);
    const unsigned* S = (const unsigned*)lds_raw + (size_t)buf * G::BUF_WORDS;
    const unsigned* qlrow = S + (16 * wave + i) * G::QLSTR;
    const unsigned* qhrow = S + G::O_QH + (16 * wave + i) * G::QHSTR;
    const f32x4 dw4 = *(const f32x4*)((const float*)S + G::O_D + 16 * wave + 4 * g);
    int iacc[NT][4];
#pragma unroll
    for (int jt = 0; jt < NT; jt++)
#pragma unroll
      for (int r = 0; r < 4; r++) iacc[jt][r] = 0;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {  // half of the super-block: 128 elements, scale groups 8h .. 8h + 7
      // the 8 group scales of this half for the four rows this lane's accumulators belong to (two words per row)
      unsigned sc_lo[4], sc_hi[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const unsigned long long t2 = *(const unsigned long long*)(S + G::O_SC + (16 * wave + 4 * g + r) * 4 + 2 * h);
        sc_lo[r] = (unsigned)t2;
        sc_hi[r] = (unsigned)(t2 >> 32);
      }
      const unsigned long long hw = *(const unsigned long long*)(qhrow + 8 * h + 2 * g);
#pragma unroll 2
      for (int c = 0; c < 4; c++) {  // unit (h, c): elements 128 h + 32 c + [0, 32)
        const unsigned long long lw = *(const unsigned long long*)(qlrow + 16 * h + 8 * (c & 1) + 2 * g);
        const unsigned long long nib = ((c >> 1) ? (lw >> 4) : lw) & 0x0F0F0F0F0F0F0F0Full;
        const unsigned long long top = ((hw >> (2 * c)) & 0x0303030303030303ull) << 4;
        const long A = (long)(nib | top);
        const long A0 = g < 2 ? A : 0l, A1 = g < 2 ? 0l : A;  // first / second 16-element scale group of the unit
        const int sh = 16 * (c & 1);  // scales 2c, 2c + 1 of the half: bytes (2c & 3), +1 of word c >> 1
#pragma unroll
        for (int jt = 0; jt < NT; jt++) {
          const long Bf = *(const long*)(S + G::O_BQ + (16 * jt + i) * G::BSTR + 32 * h + 8 * c + 2 * g);
          const i32x4 D0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(A0, Bf, i32x4{0, 0, 0, 0}, 0, 0, 0);
          const i32x4 D1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(A1, Bf, i32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const unsigned sw = ((c >> 1) ? sc_hi[r] : sc_lo[r]) >> sh;
            const int s0 = (int)(signed char)(sw & 0xffu), s1 = (int)(signed char)((sw >> 8) & 0xffu);
            iacc[jt][r] += __mul24(D0[r], s0) + __mul24(D1[r], s1);
          }
        }
      }
    }
    // offset term: (16 scales of row i) x (16 quant-sum parts of column i), k-slot groups 0 and 1; the others feed zeros
    const long As = g < 2 ? *(const long*)(S + G::O_SC + (16 * wave + i) * 4 + 2 * g) : 0l;
    const f32x2 dw01 = {dw4[0], dw4[1]}, dw23 = {dw4[2], dw4[3]};
#pragma unroll
    for (int jt = 0; jt < NT; jt++) {
      const long Bl = g < 2 ? *(const long*)(S + G::O_BLO + (16 * jt + i) * 4 + 2 * g) : 0l;
      const long Bh = g < 2 ? *(const long*)(S + G::O_BHI + (16 * jt + i) * 4 + 2 * g) : 0l;
      const i32x4 Dl = __builtin_amdgcn_mfma_i32_16x16x32_i8(As, Bl, i32x4{0, 0, 0, 0}, 0, 0, 0);
      const i32x4 Dh = __builtin_amdgcn_mfma_i32_16x16x32_i8(As, Bh, i32x4{0, 0, 0, 0}, 0, 0, 0);
      const float d8 = ((const float*)S)[G::O_BD + 16 * jt + i];
      const f32x2 d88 = {d8, d8};
      const f32x2 v01 = {(float)(iacc[jt][0] - 32 * (Dl[0] + 64 * Dh[0])), (float)(iacc[jt][1] - 32 * (Dl[1] + 64 * Dh[1]))};
      const f32x2 v23 = {(float)(iacc[jt][2] - 32 * (Dl[2] + 64 * Dh[2])), (float)(iacc[jt][3] - 32 * (Dl[3] + 64 * Dh[3]))};
      if (dbg != nullptr) {  // parity hook (NULL in every product launch): sum_g scale_g * dot_g and sum_g scale_g * bsum_g
        const int col = c0 + 16 * jt + i;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = r0 + 16 * wave + g * 4 + r;
          if (col < b && row < m) {
            int* o = dbg + (((size_t)col * m + row) * nsb + sb) * 2;
            o[0] = iacc[jt][r];
            o[1] = Dl[r] + 64 * Dh[r];
          }
        }
      }
      F[jt][0] += (dw01 * d88) * v01;
      F[jt][1] += (dw23 * d88) * v23;
    }
    commit(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int jt = 0; jt < NT; jt++) {
    const int col = c0 + 16 * jt + i;
    if (col >= b) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = r0 + 16 * wave + g * 4 + r;
      if (row < m) out[(size_t)col * m + row] = F[jt][r >> 1][r & 1];
    }
  }
}

// ---- Q8_K weights x Q8_K activation rows (buf_q8_k.rs:205-222) -----------------------------------------------------------
// The cheapest member of the family: one f32 scale per 256-element super-block on either side, so the eight MFMAs of a
// super-block chain into ONE integer accumulator (|sum| <= 256 * 127^2 < 2^23) and the scaling -- sumf += (sumi as f32 *
// d_w) * d_x, in super-block order: the scalar reference bit for bit -- happens once per 256 elements.
struct GemmGeo8K {
  static constexpr int NT = 2, CW = 32, STR = 68;  // 256 B + 16 B pad per row / column
  static constexpr int O_B = 64 * STR, O_AD = O_B + CW * STR, O_BD = O_AD + 64, BUF_WORDS = O_BD + CW;
  static constexpr int LDS_BYTES = 2 * BUF_WORDS * 4;
};
__global__ __launch_bounds__(256) void k_gemm_mfma_q8k(const i32x4* __restrict__ wq, const float* __restrict__ wd,
                                                       const char* __restrict__ act, size_t act_stride, size_t off_d,
                                                       float* __restrict__ out, int m, int nsb, int b, int row_tiles) {
  using G = GemmGeo8K;
  constexpr int NT = G::NT, CW = G::CW;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  int rt, ct;
  {
    const int col_tiles = (int)gridDim.x / row_tiles;
    if ((row_tiles & 7) == 0) {
      const int x = (int)blockIdx.x & 7, j = (int)blockIdx.x >> 3;
      ct = j % col_tiles;
      rt = (j / col_tiles) * 8 + x;
    } else {
      rt = (int)blockIdx.x % row_tiles;
      ct = (int)blockIdx.x / row_tiles;
    }
  }
  const int r0 = rt * 64, c0 = ct * CW;
  i32x4 ra[4], rb[2];
  float rdw = 0.f, rd8 = 0.f;
  auto fetch = [&](int sb) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int t = tid + 256 * u, row = t >> 4, pc = t & 15;
      const int grow = r0 + row < m ? r0 + row : m - 1;
      ra[u] = __builtin_nontemporal_load(wq + ((size_t)grow * nsb + sb) * 16 + pc);
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int t = tid + 256 * u, col = t >> 4, pc = t & 15;
      const int gcol = c0 + col < b ? c0 + col : b - 1;
      rb[u] = *((const i32x4*)(act + (size_t)gcol * act_stride) + (size_t)sb * 16 + pc);
    }
    if (tid < 64) {
      const int grow = r0 + tid < m ? r0 + tid : m - 1;
      rdw = wd[(size_t)grow * nsb + sb];
    }
    if (tid < CW) {
      const int gcol = c0 + tid < b ? c0 + tid : b - 1;
      rd8 = ((const float*)(act + (size_t)gcol * act_stride + off_d))[sb];
    }
  };
  auto commit = [&](int buf) {
    unsigned* S = (unsigned*)lds_raw + (size_t)buf * G::BUF_WORDS;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int t = tid + 256 * u;
      *(i32x4*)(S + (t >> 4) * G::STR + (t & 15) * 4) = ra[u];
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int t = tid + 256 * u;
      *(i32x4*)(S + G::O_B + (t >> 4) * G::STR + (t & 15) * 4) = rb[u];
    }
    if (tid < 64) ((float*)S)[G::O_AD + tid] = rdw;
    if (tid < CW) ((float*)S)[G::O_BD + tid] = rd8;
  };
  f32x2 F[NT][2];
#pragma unroll
  for (int jt = 0; jt < NT; jt++) F[jt][0] = F[jt][1] = f32x2{0.0f, 0.0f};
  fetch(0);
  commit(0);
  __syncthreads();
  for (int sb = 0; sb < nsb; sb++) {
    const int buf = sb & 1;
    fetch(sb + 1 < nsb ? sb + 1 : sb);
    const unsigned* S = (const unsigned*)lds_raw + (size_t)buf * G::BUF_WORDS;
    const unsigned* arow = S + (16 * wave + i) * G::STR + 2 * g;
    i32x4 D[NT];
#pragma unroll
    for (int jt = 0; jt < NT; jt++) D[jt] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const long A = *(const long*)(arow + 8 * j);
#pragma unroll
      for (int jt = 0; jt < NT; jt++) {
        const long Bf = *(const long*)(S + G::O_B + (16 * jt + i) * G::STR + 8 * j + 2 * g);
        D[jt] = __builtin_amdgcn_mfma_i32_16x16x32_i8(A, Bf, D[jt], 0, 0, 0);
      }
    }
    const f32x4 dw4 = *(const f32x4*)((const float*)S + G::O_AD + 16 * wave + 4 * g);
    const f32x2 dw01 = {dw4[0], dw4[1]}, dw23 = {dw4[2], dw4[3]};
#pragma unroll
    for (int jt = 0; jt < NT; jt++) {
      const float d8 = ((const float*)S)[G::O_BD + 16 * jt + i];
      const f32x2 d88 = {d8, d8};
      const f32x2 c01 = {(float)D[jt][0], (float)D[jt][1]}, c23 = {(float)D[jt][2], (float)D[jt][3]};
      F[jt][0] += (c01 * dw01) * d88;
      F[jt][1] += (c23 * dw23) * d88;
    }
    commit(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int jt = 0; jt < NT; jt++) {
    const int col = c0 + 16 * jt + i;
    if (col >= b) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = r0 + 16 * wave + g * 4 + r;
      if (row < m) out[(size_t)col * m + row] = F[jt][r >> 1][r & 1];
    }
  }
}

// returns false when the shape / format is not covered (the caller falls back to one GEMV per batch row)
bool launch_gemm_mfma(crabml_hip_device* dev, const crabml_hip_buf* w, size_t m, size_t k, const void* act, size_t b, float* out,
                      crabml_hip_device::ProfRec* rec, int* dbg, bool fused_add) {
  if (w->dtype != CRABML_HIP_Q4_0 && w->dtype != CRABML_HIP_Q8_0 && w->dtype != CRABML_HIP_Q4_K && w->dtype != CRABML_HIP_Q6_K &&
      w->dtype != CRABML_HIP_Q4_1 && w->dtype != CRABML_HIP_Q8_K)
    return false;
  if (b < 16 || m == 0 || k % 32 != 0) return false;
  hipStream_t st = dev->stream;
  const char* wp = (const char*)w->ptr;
  if (w->dtype == CRABML_HIP_Q8_K) {
    if (k % 256 != 0) return false;
    const ActLayout alk = act_layout(CRABML_HIP_Q8_K, k);
    const int nsb = (int)(k / 256), rtl = (int)((m + 63) / 64), ctl = (int)((b + GemmGeo8K::CW - 1) / GemmGeo8K::CW);
    launch_k(st, rec, k_gemm_mfma_q8k, dim3(rtl * ctl), dim3(256), GemmGeo8K::LDS_BYTES, (const i32x4*)wp,
             (const float*)(wp + w->wl.off_scale), (const char*)act, alk.total, alk.off_d, out, (int)m, nsb, (int)b, rtl);
    return true;
  }
  if (w->dtype == CRABML_HIP_Q6_K) {
    if (k % 256 != 0) return false;
    const ActLayout alk = act_layout(CRABML_HIP_Q8_K, k);
    const int nsb = (int)(k / 256), rtl = (int)((m + 63) / 64), ctl = (int)((b + GemmGeo6::CW - 1) / GemmGeo6::CW);
    launch_k(st, rec, k_gemm_mfma_q6k, dim3(rtl * ctl), dim3(256), GemmGeo6::LDS_BYTES, wp, (size_t)w->wl.off_scale, (const char*)act,
             alk.total, alk.off_d, alk.off_aux, out, (int)m, nsb, (int)b, rtl, dbg);
    return true;
  }
  if (w->dtype == CRABML_HIP_Q4_K) {
    if (k % 256 != 0) return false;
    const ActLayout alk = act_layout(CRABML_HIP_Q8_K, k);
    const int nsb = (int)(k / 256), rtl = (int)((m + 63) / 64);
    const bool narrow_k = (size_t)rtl * ((b + 63) / 64) < (size_t)4 * dev->n_cu && b > 16;
    const int cwk = narrow_k ? 32 : 64, ctl = (int)((b + cwk - 1) / cwk);
    with_const<2, 4>(narrow_k ? 2 : 4, [&](auto nt) {
      constexpr int N = decltype(nt)::value;
      launch_k(st, rec, k_gemm_mfma_q4k<N>, dim3(rtl * ctl), dim3(256), GemmGeoK<N>::LDS_BYTES, (const i32x4*)wp, scale_plane<i32x4>(w),
               (const char*)act, alk.total, alk.off_d, alk.off_aux, alk.off_p, out, (int)m, nsb, (int)b, rtl, dbg);
    });
    return true;
  }
  const ActLayout al = act_layout(w->dtype == CRABML_HIP_Q4_1 ? CRABML_HIP_Q8_1 : CRABML_HIP_Q8_0, k);
  const int nb = (int)(k / 32);
  const int row_tiles = (int)((m + 63) / 64);
  // 64-column tiles amortize a weight tile over more batch rows; when that grid leaves the chip under-occupied
  // (m = 4096: 64 row tiles) 32-column tiles double the workgroups per CU -- the k loop is latency-bound per wave
  static const int narrow_wgs_per_cu = [] {  // tuning hook (CRABML_HIP_TEST_HOOKS=1 CRABML_HIP_GEMM_NARROW=n): default 4
    const char* e = test_hook("CRABML_HIP_GEMM_NARROW");
    const int v = e ? atoi(e) : 4;
    return v >= 0 && v <= 16 ? v : 4;
  }();
  const bool narrow = (size_t)row_tiles * ((b + 63) / 64) < (size_t)narrow_wgs_per_cu * dev->n_cu && b > 16;
  const int cw = narrow ? 32 : 64;
  const int col_tiles = (int)((b + cw - 1) / cw);
  auto launch = [&](auto f, auto n, auto fma) {  // F the block format, N the column tiles per workgroup, FMA the fused block term
    constexpr int F = decltype(f)::value, N = decltype(n)::value;
    launch_k(st, rec, k_gemm_mfma<F, N, decltype(fma)::value>, dim3(row_tiles * col_tiles), dim3(256), GemmGeo<F, N>::LDS_BYTES, wp,
             scale_plane<unsigned short>(w), (const char*)act, al.total, al.off_d, al.off_aux, out, (int)m, nb, (int)b, row_tiles);
  };
  // the fused block term exists for Q4_0 / Q8_0 only; a Q4_1 launch with fused_add takes the plain form.  Each with_const ranges over
  // exactly the formats of its form, so no other k_gemm_mfma is instantiated.
  if (fused_add && !dev->strict_order && w->dtype != CRABML_HIP_Q4_1)
    with_const<CRABML_HIP_Q4_0, CRABML_HIP_Q8_0>((int)w->dtype, [&](auto f) {
      with_const<2, 4>(narrow ? 2 : 4, [&](auto n) { launch(f, n, std::true_type{}); });
    });
  else
    with_const<CRABML_HIP_Q4_0, CRABML_HIP_Q8_0, CRABML_HIP_Q4_1>((int)w->dtype, [&](auto f) {
      with_const<2, 4>(narrow ? 2 : 4, [&](auto n) { launch(f, n, std::false_type{}); });
    });
  return true;
}

}  // namespace crabml_hip
