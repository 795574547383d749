// sampler.hpp -- temperature / top-p sampling on the device: Llama2Sampler::sample with temperature > 0
// (crabml-llama2/src/sampler.rs:28-107), the path the CLI takes by default (--temperature 1.0 --probability 0.9).
//
//   x[i] /= T;  max = fold(NaN, f32::max);  e[i] = exp_f32_cached(x[i] - max);  p[i] = e[i] / sum(e, index order)
//   sample_topp (also for topp >= 1: sample_multi's result is discarded, sampler.rs:46-49):
//     candidates p[i] >= (1 - topp) / (n - 1), stably sorted ASCENDING by p; cumulative += p in that order until it
//     exceeds topp (that element included); r = coin * cumulative; the first element whose running cdf exceeds r wins,
//     prob_index[last_idx] if none does.
//
// Every e[i] is an f16 value in [0, 1] (the exp table's output), so p is a strictly increasing function of the 16-bit
// pattern of e: the stable ascending sort IS a histogram over the keys 0x0000 .. 0x3C00 walked in ascending key order,
// ascending index inside a key.  No comparison sort:
//   k_sample_max    SAMPLE_BLOCKS workgroups: block maxima of x / T
//   k_sample_keys   SAMPLE_BLOCKS workgroups: the global max, the key of every element (2 B each), the key histogram
//   k_sample_pick   one workgroup: sum, cutoff, the cumulative walk, r, the cdf walk -> (key, occurrence) -> index;
//                   clears the histogram for the next step and advances token / pos / step / serial like k_argmax_step
// Strict-order device: the softmax sum runs in index order and both walks add p element by element in sorted order, so
// the token is the reference's bit for bit.  Fast device: the sums are per-bin products count * p and a workgroup scan
// (DESIGN.md 2.2 states the deviation and its bound).
// Keys outside [0, 0x3C00] (a NaN or +inf logit, an overflowing x / T) and an empty nucleus (the reference panics on both)
// raise the fault word to SAMPLE_FAULT and emit token 0.
#pragma once
#include "devutil.hpp"

namespace crabml_hip {

#define SAMPLE_BLOCKS 128
#define SAMPLE_BINS 0x3C01              // keys 0x0000 .. 0x3C00: e in [0, 1]
#define SAMPLE_HIST (SAMPLE_BINS + 1)   // + one counter of keys outside [0, 1]
#define SAMPLE_FAULT 3                  // fault word value (1: norm gather, 2: tensor-parallel poll)
#define SAMPLE_PICK_THREADS 1024
#define SAMPLE_BINS_PER_THREAD 16       // 1024 x 16 >= SAMPLE_BINS

// the sampler's view of the decode state: where the coin comes from and what it advances
struct SampleStep {
  const float* par;    // {temperature, topp}
  const float* coins;  // coins[*step]
  int* token;
  int* pos;
  int* step;
  int* serial;
  unsigned* out_tokens;
  int out_cap;
  int* fault;
};

__device__ __forceinline__ float sample_wave_max(float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}

// block maxima of x / T (fmaxf ignores a NaN operand, as f32::max does)
__global__ __launch_bounds__(256) void k_sample_max(const float* __restrict__ x, int n, const float* __restrict__ par,
                                                    float* __restrict__ bmax) {
  __shared__ float s[4];
  const float T = par[0];
  const int per = (n + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  float m = -INFINITY;
  for (int i = lo + threadIdx.x; i < hi; i += 256) m = fmaxf(m, x[i] / T);  // a true division (sampler.rs:36)
  m = sample_wave_max(m);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) bmax[blockIdx.x] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}

// keys = f16 bits of exp_f32_cached(x / T - max) = exp_tab[f16_rne(x / T - max)]; histogram in LDS, flushed with atomics
__global__ __launch_bounds__(256) void k_sample_keys(const float* __restrict__ x, int n, const float* __restrict__ par,
                                                     const float* __restrict__ bmax, int nb, const unsigned short* __restrict__ exp_tab,
                                                     unsigned short* __restrict__ keys, unsigned* __restrict__ hist) {
  __shared__ unsigned h[SAMPLE_HIST];
  __shared__ float s_m;
  for (int b = threadIdx.x; b < SAMPLE_HIST; b += 256) h[b] = 0u;
  if (threadIdx.x < 64) {
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += 64) m = fmaxf(m, bmax[i]);
    m = sample_wave_max(m);
    if (threadIdx.x == 0) s_m = m;
  }
  __syncthreads();
  const float T = par[0], M = s_m;
  const int per = (n + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const float v = x[i] / T;
    const unsigned short k = exp_tab[f2h(v - M)];
    keys[i] = k;
    atomicAdd(&h[k <= 0x3C00 ? k : SAMPLE_BINS], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < SAMPLE_HIST; b += 256)
    if (h[b] != 0u) atomicAdd(&hist[b], h[b]);
}

__device__ __forceinline__ float sample_readlane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// strict walk (wave 0, all lanes in step): the candidates in ascending key order, one f32 addition per element (the
// reference's loops, sampler.rs:88-104).  Stops at the first element whose running sum exceeds `target` (returns true) or
// after element (lb, lj); (ob, oj) = the element it stopped at, -1 if there was none.
__device__ __forceinline__ bool sample_walk_strict(const unsigned* s_cnt, float sum, float cutoff, float target, int lb, int lj, int& ob, int& oj,
                                   float& cum) {
  const int lane = threadIdx.x & 63;
  cum = 0.f;
  ob = -1;
  oj = -1;
  for (int base = 0; base <= lb; base += 64) {
    const int b = base + lane;
    const unsigned c = b < SAMPLE_BINS ? s_cnt[b] : 0u;
    const float p = h2f((unsigned short)min(b, 0x3C00)) / sum;
    unsigned long long mask = __ballot(c != 0u && p >= cutoff && b <= lb);
    while (mask) {
      const int k = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int bb = base + k;
      const float pp = sample_readlane_f(p, k);
      const int nj = bb == lb ? lj + 1 : (int)__builtin_amdgcn_readlane((int)c, k);
      for (int j = 0; j < nj; j++) {
        cum += pp;
        if (cum > target) {
          ob = bb;
          oj = j;
          return true;
        }
      }
      ob = bb;
      oj = nj - 1;
    }
  }
  return false;
}

// fast walk (every thread): m[] = the masses count * p of this thread's bins, pre = the scan of the masses before them.
// The first element whose running sum exceeds `target` (true), else the last candidate element; candidates beyond (lb, lj)
// are never returned.  Reduced through s_hit.
__device__ __forceinline__ void sample_walk_fast(const float* m, const float* p, const unsigned* cnt, float pre, float target, int lb, int lj,
                                 int* s_hit, int& ob, int& oj, float& cum, float* s_cum) {
  const int b0 = threadIdx.x * SAMPLE_BINS_PER_THREAD;
  if (threadIdx.x == 0) {
    s_hit[0] = 0x7fffffff;
    s_hit[1] = -1;
  }
  __syncthreads();
  float run = pre;
  int hit = -1, lastb = -1;
#pragma unroll
  for (int k = 0; k < SAMPLE_BINS_PER_THREAD; k++) {
    const int b = b0 + k;
    if (m[k] > 0.f && b <= lb) {
      if (hit < 0 && run + m[k] > target) hit = b;
      lastb = b;
      run += m[k];
    }
  }
  if (hit >= 0) atomicMin(&s_hit[0], hit);
  if (lastb >= 0) atomicMax(&s_hit[1], lastb);
  __syncthreads();
  const int hb = s_hit[0];
  const bool found = hb != 0x7fffffff;
  const int bb = found ? hb : s_hit[1];
  if (bb >= 0 && bb >= b0 && bb < b0 + SAMPLE_BINS_PER_THREAD) {  // the owner of the bin finishes
    float r = pre;
    int kk = 0;
#pragma unroll
    for (int k = 0; k < SAMPLE_BINS_PER_THREAD; k++)
      if (b0 + k < bb && m[k] > 0.f && b0 + k <= lb) r += m[k];
#pragma unroll
    for (int k = 0; k < SAMPLE_BINS_PER_THREAD; k++)
      if (b0 + k == bb) kk = k;
    const int cmax = (bb == lb ? lj + 1 : (int)cnt[kk]) - 1;
    int j = cmax;
    if (found) {
      const float q = floorf((target - r) / p[kk]);
      j = q < 0.f ? 0 : q > (float)cmax ? cmax : (int)q;
    }
    s_hit[2] = j;
    *s_cum = r + (float)(j + 1) * p[kk];
  }
  __syncthreads();
  ob = bb;
  oj = bb >= 0 ? s_hit[2] : -1;
  cum = *s_cum;
  __syncthreads();
}

template <bool STRICT>
__global__ __launch_bounds__(SAMPLE_PICK_THREADS) void k_sample_pick(const unsigned short* __restrict__ keys, int n,
                                                                     unsigned* __restrict__ hist, SampleStep s) {
  __shared__ unsigned s_cnt[STRICT ? SAMPLE_BINS : 1];
  __shared__ float s_red[16];
  __shared__ int s_hit[4];
  __shared__ int s_wc[16];
  __shared__ float s_sum, s_cum;
  __shared__ int s_sel[4];  // {bin, occurrence, token, fault}
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float topp = s.par[1];
  const int step = *s.step;
  const float coin = s.coins[step < s.out_cap ? step : s.out_cap - 1];
  const int b0 = tid * SAMPLE_BINS_PER_THREAD;

  // the histogram: to registers (and LDS on the strict device); cleared for the next step
  unsigned cnt[SAMPLE_BINS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < SAMPLE_BINS_PER_THREAD; k++) cnt[k] = b0 + k < SAMPLE_BINS ? hist[b0 + k] : 0u;
  if constexpr (STRICT) {
#pragma unroll
    for (int k = 0; k < SAMPLE_BINS_PER_THREAD; k++)
      if (b0 + k < SAMPLE_BINS) s_cnt[b0 + k] = cnt[k];
  }
  if (tid == 0) {
    s_sel[3] = hist[SAMPLE_BINS] != 0u;  // a key outside [0, 1]: NaN / +inf in the logits
    s_sel[0] = -1;
  }
  __syncthreads();
  for (int b = tid; b < SAMPLE_HIST; b += SAMPLE_PICK_THREADS) hist[b] = 0u;

  // softmax denominator (sampler.rs:121-125)
  if constexpr (STRICT) {
    if (tid == 0) {
      float sum = 0.f;
      int i = 0;
      const bool a16 = ((size_t)keys & 15) == 0;
      if (a16) {
#pragma unroll 4
        for (; i + 8 <= n; i += 8) {
          const uint4 q = *(const uint4*)(keys + i);
          sum += h2f((unsigned short)(q.x & 0xffff));
          sum += h2f((unsigned short)(q.x >> 16));
          sum += h2f((unsigned short)(q.y & 0xffff));
          sum += h2f((unsigned short)(q.y >> 16));
          sum += h2f((unsigned short)(q.z & 0xffff));
          sum += h2f((unsigned short)(q.z >> 16));
          sum += h2f((unsigned short)(q.w & 0xffff));
          sum += h2f((unsigned short)(q.w >> 16));
        }
      }
      for (; i < n; i++) sum += h2f(keys[i]);
      s_sum = sum;
    }
  } else {
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < SAMPLE_BINS_PER_THREAD; k++)
      if (cnt[k]) part += (float)cnt[k] * h2f((unsigned short)(b0 + k));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) s_red[w] = part;
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int i = 0; i < 16; i++) t += s_red[i];
      s_sum = t;
    }
  }
  __syncthreads();
  const float sum = s_sum;
  const float cutoff = (1.0f - topp) / (float)(n - 1);  // sampler.rs:75

  if constexpr (STRICT) {
    if (w == 0) {
      int lb, lj, cb, cj;
      float cum, cdf;
      sample_walk_strict(s_cnt, sum, cutoff, topp, SAMPLE_BINS, 0, lb, lj, cum);
      if (lb >= 0) {
        const float r = coin * cum;
        if (!sample_walk_strict(s_cnt, sum, cutoff, r, lb, lj, cb, cj, cdf)) {
          cb = lb;  // rounding: prob_index[last_idx]
          cj = lj;
        }
        if (lane == 0) {
          s_sel[0] = cb;
          s_sel[1] = cj;
        }
      }
    }
  } else {
    float p[SAMPLE_BINS_PER_THREAD], m[SAMPLE_BINS_PER_THREAD];
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < SAMPLE_BINS_PER_THREAD; k++) {
      p[k] = h2f((unsigned short)min(b0 + k, 0x3C00)) / sum;
      m[k] = cnt[k] != 0u && p[k] >= cutoff ? (float)cnt[k] * p[k] : 0.f;
      // a candidate bin of p = 0 (topp >= 1) adds nothing; keep it out of the walk
      tot += m[k];
    }
    // exclusive scan of the per-thread masses
    float inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) s_red[w] = inc;
    __syncthreads();
    float wpre = 0.f;
    for (int i = 0; i < w; i++) wpre += s_red[i];
    const float pre = wpre + inc - tot;
    int lb, lj, cb, cj;
    float cum, cdf;
    sample_walk_fast(m, p, cnt, pre, topp, SAMPLE_BINS, 0, s_hit, lb, lj, cum, &s_cum);
    if (lb >= 0) {
      const float r = coin * cum;
      sample_walk_fast(m, p, cnt, pre, r, lb, lj, s_hit, cb, cj, cdf, &s_cum);
      if (tid == 0) {
        s_sel[0] = cb;
        s_sel[1] = cj;
      }
    }
  }
  __syncthreads();

  // the (occurrence)-th index, in index order, whose key is `bin`: per-wave counts over contiguous segments, then one wave
  // rescans the segment that holds it; 8 independent loads per lane in flight (a wave walks ~2k keys)
  const int bin = s_sel[0], occ = s_sel[1];
  int token = -1;
  if (bin >= 0) {
    constexpr int U = 8;
    const unsigned short kb = (unsigned short)bin;  // <= 0x3C00: never the 0xFFFF of a lane past the end
    const int seg = ((n + 15) / 16 + 64 * U - 1) / (64 * U) * (64 * U);
    const int lo = w * seg, hi = min(n, lo + seg);
    int c = 0;
    for (int i0 = lo; i0 < hi; i0 += 64 * U) {
      unsigned short kv[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int i = i0 + u * 64 + lane;
        kv[u] = i < hi ? keys[i] : (unsigned short)0xFFFF;
      }
#pragma unroll
      for (int u = 0; u < U; u++) c += __popcll(__ballot(kv[u] == kb));
    }
    if (lane == 0) s_wc[w] = c;
    __syncthreads();
    int before = 0, ww = 0;
    for (; ww < 16; ww++) {
      if (before + s_wc[ww] > occ) break;
      before += s_wc[ww];
    }
    if (w == ww) {
      int run = before;
      bool done = false;
      for (int i0 = lo; i0 < hi && !done; i0 += 64 * U) {
        unsigned short kv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int i = i0 + u * 64 + lane;
          kv[u] = i < hi ? keys[i] : (unsigned short)0xFFFF;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          unsigned long long mask = __ballot(kv[u] == kb);
          const int pc = __popcll(mask);
          if (!done && run + pc > occ) {
            for (int k = occ - run; k > 0; k--) mask &= mask - 1;
            if (lane == 0) s_sel[2] = i0 + u * 64 + __builtin_ctzll(mask);
            done = true;
          }
          run += pc;
        }
      }
    }
    __syncthreads();
    if (ww < 16) token = s_sel[2];
  }
  if (tid == 0) {
    const bool bad = s_sel[3] != 0 || token < 0 || token >= n;
    if (bad) {
      token = 0;
      *s.fault = SAMPLE_FAULT;
    }
    *s.token = token;
    const int st = *s.step;
    if (st < s.out_cap) s.out_tokens[st] = (unsigned)token;
    *s.step = st + 1;
    *s.pos = *s.pos + 1;
    *s.serial = *s.serial + 1;
  }
}

}  // namespace crabml_hip
