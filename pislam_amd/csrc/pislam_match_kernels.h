// Brute-force Hamming matching of binary descriptors (README.md:125-128 names
// matching as the consumer of the front-end's output — the reference ships no matcher, so the
// semantics are this library's own: include/pislam_hip.h).
//
// For every query descriptor: the train descriptor with the smallest Hamming distance (ties -> the
// smallest train index) and the smallest distance among all OTHER train descriptors (for a ratio
// test).  One lane = one query held in registers; the train descriptor of an iteration is the same
// for the whole wave, so it is fetched with SCALAR loads (s_load_dwordx8) and XOR-ed as an SGPR
// operand; popcount-accumulate is one instruction (v_bcnt_u32_b32).  best / second are tracked on
// the packed key dist << 16 | index with one max and two mins.  Popcount (VALU issue) bound:
// ~21 instructions per (query, train) pair per wave of 64 queries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace pm {

constexpr int MAX_WORDS = 16;

// ---------------------------------------------------------------------------
// Pieces the matchers, the bag-of-words kernels (pislam_bow_kernels.h) and the key-frame database
// (pislam_bowdb_kernels.h) share: the workgroup scan, the LDS counting sort of the two index kernels, and the
// (best, second) bookkeeping of the match kernels.
// ---------------------------------------------------------------------------

// Exclusive scan of one value per thread over the THREADS threads of the workgroup: returns the sum over the threads
// below this one, *total = the sum over all.  wave_sum: LDS [THREADS / 64].  The one barrier lies between writing and
// reading wave_sum; a caller that writes wave_sum again afterwards puts its own barrier in between.
template <int THREADS>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wave_sum, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if ((int)lane >= d) incl += o;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t run = incl - v, tot = 0;
  for (uint32_t w = 0; w < (uint32_t)(THREADS / 64); w++) {
    const uint32_t x = wave_sum[w];
    if (w < wave) run += x;
    tot += x;
  }
  *total = tot;
  return run;
}

// Counting sort of entries 0 .. n - 1 into nbins bins by one workgroup of THREADS threads: histogram with LDS atomics,
// exclusive scan (every thread sums a contiguous chunk of bins, block_scan over the chunk sums), then the scatter.
// hist: LDS [>= nbins], wave_sum: LDS [THREADS / 64], off: the pair's offset row in global memory, off[c] = first slot
// of bin c and off[nbins] = entries indexed.  bin_of(j) is the bin of entry j, negative for an entry that is not
// indexed; it is evaluated in the count pass and again in the scatter pass, where place(slot, j) follows it at once in
// the same thread (so place may use what bin_of left behind).  Slot order inside a bin varies between runs.
template <int THREADS, class BinOf, class Place>
__device__ __forceinline__ void lds_counting_sort(uint32_t nbins, uint32_t n, uint32_t *hist, uint32_t *wave_sum,
                                                  uint32_t *__restrict__ off, BinOf &&bin_of, Place &&place) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t c = tid; c < nbins; c += THREADS) hist[c] = 0;
  __syncthreads();
  for (uint32_t j = tid; j < n; j += THREADS) {
    const int32_t c = bin_of(j);
    if (c >= 0) atomicAdd(&hist[c], 1u);
  }
  __syncthreads();
  const uint32_t chunk = (nbins + THREADS - 1) / THREADS;
  const uint32_t c0 = min(tid * chunk, nbins), c1 = min(c0 + chunk, nbins);
  uint32_t s = 0, total;
  for (uint32_t c = c0; c < c1; c++) s += hist[c];
  uint32_t run = block_scan<THREADS>(s, wave_sum, &total);
  for (uint32_t c = c0; c < c1; c++) {
    const uint32_t v = hist[c];
    hist[c] = run;
    run += v;
  }
  if (tid == 0) off[nbins] = total;
  __syncthreads();
  for (uint32_t c = tid; c < nbins; c += THREADS) off[c] = hist[c];
  __syncthreads();
  for (uint32_t j = tid; j < n; j += THREADS) {
    const int32_t c = bin_of(j);
    if (c >= 0) place(atomicAdd(&hist[c], 1u), j);       // hist[c] is the next free slot of bin c
  }
}

// The two smallest of the keys dist << 16 | index seen so far, 0xffffffff for "none" (keys are at most
// 256 << 16 | 65534: never the sentinel).  Keys are unique per train index, so neither depends on the visit order.
__device__ __forceinline__ void pair_push(uint32_t &best, uint32_t &second, uint32_t key) {
  second = min(second, max(best, key));
  best = min(best, key);
}

// Merges the pair (ob, os) of a disjoint set of entries into (best, second).
__device__ __forceinline__ void pair_merge(uint32_t &best, uint32_t &second, uint32_t ob, uint32_t os) {
  second = min(min(second, os), max(best, ob));
  best = min(best, ob);
}

// Merges the pairs of the LPQ adjacent lanes of a query (they saw disjoint entries): every one of them gets the result.
template <int LPQ>
__device__ __forceinline__ void pair_merge_lanes(uint32_t &best, uint32_t &second) {
#pragma unroll
  for (int s = 1; s < LPQ; s <<= 1) {
    const uint32_t ob = __shfl_xor(best, s, 64), os = __shfl_xor(second, s, 64);
    pair_merge(best, second, ob, os);
  }
}

// Output slot o of a guided matcher: "none" becomes index -1 and distance 0xffffffff.
__device__ __forceinline__ void store_match(size_t o, uint32_t best, int32_t *__restrict__ idx, uint32_t *__restrict__ dist) {
  idx[o] = best == 0xffffffffu ? -1 : (int32_t)(best & 0xffffu);
  dist[o] = best == 0xffffffffu ? 0xffffffffu : best >> 16;
}
__device__ __forceinline__ void store_match(size_t o, uint32_t best, uint32_t second, int32_t *__restrict__ idx,
                                            uint32_t *__restrict__ dist, uint32_t *__restrict__ dist2) {
  store_match(o, best, idx, dist);
  dist2[o] = second == 0xffffffffu ? 0xffffffffu : second >> 16;
}

// The query descriptor of a lane: the WORDS dwords at p, zeros for a lane without a query (p null).
template <int WORDS>
__device__ __forceinline__ void load_query(uint32_t (&qd)[WORDS], const uint32_t *__restrict__ p) {
#pragma unroll
  for (int w = 0; w < WORDS; w++) qd[w] = 0;
  if (p) {
#pragma unroll
    for (int w = 0; w < WORDS; w++) qd[w] = p[w];
  }
}

constexpr int QPW = 64;                // queries per workgroup pass (one per lane; the waves split the train set)
constexpr int SPLIT = 8;               // waves per workgroup = interleaved slices of the train set
constexpr int MAX_GRID_X = 16;         // query tiles per pair in flight; a workgroup loops over further tiles

// grid (min(ceil(max_q / 64), 16), batch), 64 * SPLIT threads; descriptors [batch][stride][WORDS];
// counts may be null (then nq / nt apply to every pair).  Train sets larger than 65535 are rejected
// by the host.  All waves of a workgroup hold the same 64 queries (one per lane, in registers) and
// scan interleaved slices of the train set (a front-end batch only has ~1000 queries per pair:
// SPLIT x the waves in flight), two descriptors per iteration; the partial (best, second) pairs are
// merged through LDS.  The train descriptor of an iteration is wave-uniform and is fetched with
// SCALAR loads (s_load_dwordx8, XOR-ed as an SGPR operand).  Measured alternatives for that operand:
// LDS tiles read back with broadcast ds_read_b128 (+11 %), per-lane vector loads of the same address
// (+67 %, bound by the L1 return path).  SMEM returns out of order (only lgkmcnt(0) can wait for it),
// so the loads cannot be software-pipelined inside a wave; the other waves of the SIMD cover them.
template <int WORDS>
__global__ __launch_bounds__(QPW *SPLIT) void k_match(const uint32_t *__restrict__ q, const uint32_t *__restrict__ qcount,
                                                      size_t q_stride, uint32_t nq_all, const uint32_t *__restrict__ t,
                                                      const uint32_t *__restrict__ tcount, size_t t_stride,
                                                      uint32_t nt_all, uint32_t cap_q, uint32_t cap_t,
                                                      int32_t *__restrict__ idx, uint32_t *__restrict__ dist,
                                                      uint32_t *__restrict__ dist2, size_t out_stride) {
  __shared__ uint32_t sh_best[SPLIT][QPW], sh_second[SPLIT][QPW];
  const int b = blockIdx.y;
  const uint32_t nq = min(qcount ? qcount[b] : nq_all, cap_q);
  const uint32_t nt = min(tcount ? tcount[b] : nt_all, cap_t);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t *tp = t + (size_t)b * t_stride;
  for (uint32_t q0 = blockIdx.x * (uint32_t)QPW; q0 < nq; q0 += gridDim.x * (uint32_t)QPW) {
    const uint32_t i = q0 + lane;
    const uint32_t *qp = q + (size_t)b * q_stride + (size_t)min(i, nq - 1) * WORDS;
    uint32_t qd[WORDS];
#pragma unroll
    for (int k = 0; k < WORDS; k++) qd[k] = qp[k];
    uint32_t best = 0xffffffffu, second = 0xffffffffu;
    uint32_t j = wave;
    for (; j + SPLIT < nt; j += 2 * SPLIT) {             // two train descriptors per iteration: j and j + SPLIT
      const uint32_t *t0 = tp + (size_t)j * WORDS, *t1 = t0 + SPLIT * WORDS;   // wave-uniform -> scalar loads
      uint32_t d0 = 0, d1 = 0;
#pragma unroll
      for (int k = 0; k < WORDS; k++) {
        d0 += (uint32_t)__popc(qd[k] ^ t0[k]);
        d1 += (uint32_t)__popc(qd[k] ^ t1[k]);
      }
      pair_push(best, second, (d0 << 16) | j);
      pair_push(best, second, (d1 << 16) | (j + SPLIT));
    }
    if (j < nt) {
      const uint32_t *t0 = tp + (size_t)j * WORDS;
      uint32_t d0 = 0;
#pragma unroll
      for (int k = 0; k < WORDS; k++) d0 += (uint32_t)__popc(qd[k] ^ t0[k]);
      pair_push(best, second, (d0 << 16) | j);
    }
    sh_best[wave][lane] = best;
    sh_second[wave][lane] = second;
    __syncthreads();
    if (wave == 0 && i < nq) {
#pragma unroll
      for (int w = 1; w < SPLIT; w++) pair_merge(best, second, sh_best[w][lane], sh_second[w][lane]);
      const size_t o = (size_t)b * out_stride + i;
      idx[o] = nt ? (int32_t)(best & 0xffffu) : -1;
      dist[o] = nt ? best >> 16 : 0xffffffffu;
      dist2[o] = nt > 1 ? second >> 16 : 0xffffffffu;
    }
    __syncthreads();                                     // sh_best / sh_second are reused by the next tile
  }
}

// ---------------------------------------------------------------------------
// The same matcher on the matrix cores (gfx950 v_mfma_i32_32x32x32_i8).  All-pairs Hamming distance is a
// GEMM over bits: with the train bits as 0/1 bytes (A, rows) and the query bits as +1/-1 bytes (B, columns),
//   C[j][i] = sum_k t_jk * (2 q_ik - 1) = 2 popc(t_j & q_i) - popc(t_j),   dist(i, j) = popc(q_i) - C[j][i],
// so one 32x32x32 MFMA per descriptor word covers 32 train x 32 query descriptors, and popc(q_i) is a per-lane
// constant (the C layout gives every lane ONE query column: col = lane & 31, rows (reg & 3) + 8 (reg >> 2) +
// 4 (lane >> 5)).  A and B fragments use the same lane -> (index, k-half) rule, so only "row / col = lane & 31,
// the two lane halves split k" is assumed of the operand layout, not the order of k inside a half.
//
// One wave = 32 queries (B fragments of all words stay in registers), sweeping the train set in tiles of 32; a
// tile's raw words are expanded to bytes through a 256-entry LDS table (8 bits -> 8 bytes, two ds_read_b64 per
// word), the next tile's words are loaded while the MFMAs run.  Epilogue per C element: key = row - (C << 16)
// (v_mad_i32_i24), second = med3(best, second, key), best = min(best, key) on tile-local keys; the tile's pair is
// shifted by its first train index and merged into the running pair; popc(q) << 16 is added once at the end.
// Keys order exactly like the VALU kernel's dist << 16 | index, so the results are identical (ties -> the
// smallest train index).  ~3.5 VALU per (query, train) pair per wave instead of ~21: batch 256 x 981 x 981 pairs in
// 0.09 ms against 0.15 ms (tools/probes/match_probe.hip), VALU issue and the MFMA pipe sharing the time evenly.
// ---------------------------------------------------------------------------
typedef int mf_v4i __attribute__((ext_vector_type(4)));
typedef int mf_v16i __attribute__((ext_vector_type(16)));
constexpr int MF_WAVES = 4;            // waves per workgroup: 4 x 32 queries per pass
constexpr int MF_Q = 32 * MF_WAVES;
constexpr int32_t MF_BIG = 0x7ff00000; // "no candidate": larger than any key, small enough to add a train index to


// Pins a prefetched register array at this point of the program: the compiler has to have the loads issued
// before and their values complete here (it otherwise sinks a prefetch down to its first use in the NEXT
// iteration, and every tile then waits out a full global-load latency).
template <int WORDS>
__device__ __forceinline__ void mf_pin(uint32_t (&d)[WORDS]) {
  if constexpr (WORDS == 8)
    asm volatile("" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]), "+v"(d[7]));
  else if constexpr (WORDS == 4)
    asm volatile("" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]));
  else if constexpr (WORDS == 2)
    asm volatile("" : "+v"(d[0]), "+v"(d[1]));
  else
    asm volatile("" : "+v"(d[0]));
}

template <int WORDS>
__global__ __launch_bounds__(64 * MF_WAVES) void k_match_mfma(const uint32_t *__restrict__ q, const uint32_t *__restrict__ qcount,
                                                              size_t q_stride, uint32_t nq_all, const uint32_t *__restrict__ t,
                                                              const uint32_t *__restrict__ tcount, size_t t_stride,
                                                              uint32_t nt_all, uint32_t cap_q, uint32_t cap_t,
                                                              int32_t *__restrict__ idx, uint32_t *__restrict__ dist,
                                                              uint32_t *__restrict__ dist2, size_t out_stride) {
  __shared__ uint2 tab[256];                             // 8 bits -> 8 bytes of 0 / 1 (bit k -> byte k)
  const int b = blockIdx.y;
  const uint32_t nq = min(qcount ? qcount[b] : nq_all, cap_q);
  if (blockIdx.x * (uint32_t)MF_Q >= nq) return;         // (the grid is sized for the capacity, not for the counts)
  {
    const uint32_t e = threadIdx.x;
    auto spread = [](uint32_t n) {                       // 4 bits -> 4 bytes
      uint32_t v = n | (n << 7);
      v |= v << 14;
      return v & 0x01010101u;
    };
    tab[e] = make_uint2(spread(e & 15u), spread(e >> 4));
  }
  __syncthreads();
  const uint32_t nt = min(tcount ? tcount[b] : nt_all, cap_t);
  const uint32_t lane = threadIdx.x & 63u, col = lane & 31u, half = lane >> 5;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t sh = 16u * half;                        // this lane half's 16 bits of every word
  const uint32_t *tp = t + (size_t)b * t_stride;
  const uint2 *tabp = tab;
  auto expand01 = [&](uint32_t w) -> mf_v4i {            // 16 bits -> 16 bytes of 0 / 1
    const uint32_t w16 = w >> sh;                        // (then the two index bytes are fixed byte selects)
    const uint2 e0 = tabp[w16 & 255u], e1 = tabp[(w16 >> 8) & 255u];
    return (mf_v4i){(int)e0.x, (int)e0.y, (int)e1.x, (int)e1.y};
  };
  auto pm1 = [](int x) -> int { return (int)((((uint32_t)x ^ 0x01010101u) * 0xfeu) | 0x01010101u); };   // 0/1 -> -1/+1 bytes
  for (uint32_t q0 = blockIdx.x * (uint32_t)MF_Q + wave * 32u; q0 < nq; q0 += gridDim.x * (uint32_t)MF_Q) {
    const uint32_t i = q0 + col;
    const uint32_t *qp = q + (size_t)b * q_stride + (size_t)min(i, nq - 1) * WORDS;
    mf_v4i bq[WORDS];
    uint32_t pq = 0;
#pragma unroll
    for (int k = 0; k < WORDS; k++) {
      const uint32_t w = qp[k];
      pq += (uint32_t)__popc(w);
      const mf_v4i e = expand01(w);
      bq[k] = (mf_v4i){pm1(e.x), pm1(e.y), pm1(e.z), pm1(e.w)};
    }
    int32_t gb = MF_BIG, gs = MF_BIG;
    // raw words of the tile in flight: loaded one tile ahead (at the top of an iteration, pinned at its bottom)
    uint32_t tw[WORDS], tn[WORDS];
    if (nt) {
      const uint32_t *t0 = tp + (size_t)min(col, nt - 1) * WORDS;
#pragma unroll
      for (int k = 0; k < WORDS; k++) tn[k] = t0[k];
    }
    // one tile of 32 train descriptors; FULL = all 32 rows exist (the tail tile masks the missing rows)
    auto tile = [&](uint32_t jt, auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
      for (int k = 0; k < WORDS; k++) tw[k] = tn[k];
      {
        const uint32_t *t1 = tp + (size_t)min(jt + 32u + col, nt - 1) * WORDS;   // (the last tile re-reads a valid row)
#pragma unroll
        for (int k = 0; k < WORDS; k++) tn[k] = t1[k];
      }
      mf_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < WORDS; k++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(expand01(tw[k]), bq[k], acc, 0, 0, 0);
      int32_t b2 = MF_BIG, s2 = MF_BIG;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int ofs = (r & 3) + 8 * (r >> 2);          // row of this accumulator register (+ 4 * half)
        int32_t lk = __mul24(acc[r], -65536) + ofs;      // v_mad_i32_i24 (|C| <= 256)
        if (!FULL && jt + (uint32_t)ofs + 4u * half >= nt) lk = MF_BIG;
        asm("v_med3_i32 %0, %1, %2, %3" : "=v"(s2) : "v"(b2), "v"(s2), "v"(lk));   // b2 <= s2: the second smallest of the three
        b2 = min(b2, lk);
      }
      const int32_t jofs = (int32_t)(jt + 4u * half);
      b2 += jofs;
      s2 += jofs;
      gs = min(min(gs, s2), max(gb, b2));
      gb = min(gb, b2);
      mf_pin<WORDS>(tn);
    };
    uint32_t jt = 0;
    for (; jt + 32u <= nt; jt += 32u) tile(jt, std::true_type{});
    if (jt < nt) tile(jt, std::false_type{});
    // the two lane halves hold the even / odd groups of four train rows of the same query
    const int32_t ob = __shfl_xor(gb, 32, 64), os = __shfl_xor(gs, 32, 64);
    gs = min(min(gs, os), max(gb, ob));
    gb = min(gb, ob);
    if (half == 0 && i < nq) {
      const size_t o = (size_t)b * out_stride + i;
      const uint32_t kb = (uint32_t)gb + (pq << 16), ks = (uint32_t)gs + (pq << 16);
      idx[o] = nt ? (int32_t)(kb & 0xffffu) : -1;
      dist[o] = nt ? kb >> 16 : 0xffffffffu;
      dist2[o] = nt > 1 ? ks >> 16 : 0xffffffffu;
    }
  }
}

// ---------------------------------------------------------------------------
// Guided window matching (include/pislam_hip.h): every position is mapped to level-0 coordinates
// through its level's Q16 scale, X = ((x - col0) * s + 32768) >> 16 (likewise Y); query i of level lq sees the train
// entries of the levels within `span` of lq whose mapped position lies within radius0[lq] of the window centre (the
// query's own mapped position, or a per-query prediction), with the outputs of k_match restricted to those candidates.
// The windowed matcher is the case of unit scales (65536: X = x - col0) and span 0.  Two launches on the context stream:
//   k_scaled_index   one workgroup per pair: each train entry goes to a cell of ITS level's grid of square cells in
//                    level-0 pixels (side chosen by the host), so a cell run holds one level and the match needs no level
//                    test; lds_counting_sort with the cell as the bin writes the pair's cell offsets and a cell-sorted
//                    copy of each entry (X << 16 | Y, original index, descriptor dwords).
//   k_match_scaled   WIN_LPQ lanes per query (the query descriptor in registers): the cell rows overlapping the window
//                    clipped to a level's mapped extent are contiguous runs of entries; the lanes of a query take every
//                    WIN_LPQ-th entry of each run, apply the exact window test, XOR-popcount and keep (best, second) on
//                    dist << 16 | index like k_match (pair_push), then merge through two xor-shuffles.  At span 0 (ONE_LEVEL) a lane
//                    walks its own level with that level's fields picked per lane; otherwise a wave-uniform loop over the
//                    plan's levels (kernel-argument loads, no per-lane indexing of the plan) walks the levels within span.
// Positions outside every level are never indexed and find no candidates.  Scatter order inside a cell varies between
// runs; the results do not: the packed key is unique per train index, so the minimum does not depend on visit order.
// ---------------------------------------------------------------------------
constexpr int WIN_MAX_LEVELS = 16;
constexpr int WIN_MAX_CELLS = 16384;   // LDS histogram of k_scaled_index (64 KiB); the host coarsens cells to fit
constexpr int WIN_INDEX_THREADS = 1024;
constexpr int WIN_THREADS = 256;       // k_match_scaled / k_match_stereo workgroup
constexpr int WIN_LPQ = 4;             // lanes per query
constexpr int WIN_QPW = WIN_THREADS / WIN_LPQ;   // queries per workgroup pass

struct alignas(16) ScaledLevel {      // (16-byte aligned: the level search fetches the rectangle with one scalar load)
  int32_t col0, row0, width, height;   // rectangle inside the stacked pyramid
  int32_t scale;                       // level-0 pixels per level pixel, Q16 (1 .. 2^20)
  int32_t ext_x, ext_y;                // largest mapped X / Y of the level (<= 65535)
  int32_t radius;                      // radius0[l]: window radius of a query on this level (level-0 pixels)
  int32_t side, ncx, base;             // grid of the level's train entries: cell side (level-0 pixels), cells per cell
                                       // row, first cell of the level in the pair's cell table
};
struct ScaledPlan {                    // passed by value (kernel arguments: a captured graph keeps its own copy)
  ScaledLevel lv[WIN_MAX_LEVELS];
  int32_t nlevels, ncells, span;       // ncells: cells of all levels (<= WIN_MAX_CELLS); span: |lq - lt| <= span
};

// A count as the window matchers read it: PISLAM_COUNT_INVALID (a pyramid the front end did not produce) is 0.
__device__ __forceinline__ uint32_t win_count(uint32_t c, size_t stride) {
  return c == 0xffffffffu ? 0u : (uint32_t)min((size_t)c, stride);
}

// Level-0 coordinate of a level-local coordinate u (unsigned 32-bit: u <= 4095 and scale <= 2^20 cannot wrap).
__device__ __forceinline__ int32_t sc_map(int32_t u, int32_t scale) {
  return (int32_t)(((uint32_t)u * (uint32_t)scale + 32768u) >> 16);
}

// The level whose rectangle holds (x, y): the loop is wave-uniform (kernel-argument loads), the fields of the level
// found are picked by selects, so no per-lane indexing of the plan (which would go through scratch).  The two range
// tests are combined with `&`: a short-circuit `&&` splits them into two branches with a scalar-load wait each.
struct ScaledHit {
  int32_t level, col0, row0, scale, ext_x, ext_y, radius, side, ncx, base;   // level -1: in no level
};
__device__ __forceinline__ ScaledHit sc_level(const ScaledPlan &P, int32_t x, int32_t y) {
  ScaledHit h{-1, 0, 0, 0, 0, 0, 0, 1, 0, 0};
  for (int l = 0; l < P.nlevels; l++) {
    const ScaledLevel L = P.lv[l];
    if (((uint32_t)(x - L.col0) < (uint32_t)L.width) & ((uint32_t)(y - L.row0) < (uint32_t)L.height)) {
      h = ScaledHit{l, L.col0, L.row0, L.scale, L.ext_x, L.ext_y, L.radius, L.side, L.ncx, L.base};
    }
  }
  return h;
}

// Cell of a packed position (x << 12 | y; score bits ignored) in its level's grid, -1 outside every level; *xy gets
// the mapped X << 16 | Y.
__device__ __forceinline__ int32_t sc_cell(const ScaledPlan &P, uint32_t k, uint32_t *xy) {
  const int32_t x = (int32_t)((k >> 12) & 0xfffu), y = (int32_t)(k & 0xfffu);
  const ScaledHit h = sc_level(P, x, y);
  if (h.level < 0) return -1;
  const int32_t X = sc_map(x - h.col0, h.scale), Y = sc_map(y - h.row0, h.scale);
  *xy = (uint32_t)X << 16 | (uint32_t)Y;
  return h.base + (Y / h.side) * h.ncx + X / h.side;
}

// grid (batch), WIN_INDEX_THREADS threads.  t_stride in entries; cell_off [batch][ncells + 1],
// ent_meta [batch][t_stride] = (X << 16 | Y, original index), ent_desc [batch][t_stride][words].
__global__ __launch_bounds__(WIN_INDEX_THREADS) void k_scaled_index(ScaledPlan P, int words, const uint32_t *__restrict__ tkp,
                                                                    const uint32_t *__restrict__ tdesc,
                                                                    const uint32_t *__restrict__ tcount, size_t t_stride,
                                                                    uint32_t *__restrict__ cell_off, uint2 *__restrict__ ent_meta,
                                                                    uint32_t *__restrict__ ent_desc) {
  __shared__ uint32_t hist[WIN_MAX_CELLS];
  __shared__ uint32_t wave_sum[WIN_INDEX_THREADS / 64];
  const int b = blockIdx.x;
  const uint32_t *kp = tkp + (size_t)b * t_stride;
  const uint32_t *dp = tdesc + (size_t)b * t_stride * words;
  uint2 *mp = ent_meta + (size_t)b * t_stride;
  uint32_t *ep = ent_desc + (size_t)b * t_stride * words;
  uint32_t xy = 0;                                       // mapped position of the entry bin_of saw last
  lds_counting_sort<WIN_INDEX_THREADS>(
      (uint32_t)P.ncells, win_count(tcount[b], t_stride), hist, wave_sum, cell_off + (size_t)b * (P.ncells + 1),
      [&](uint32_t j) { return sc_cell(P, kp[j], &xy); },
      [&](uint32_t slot, uint32_t j) {
        mp[slot] = make_uint2(xy, j);
        for (int w = 0; w < words; w++) ep[(size_t)slot * words + w] = dp[(size_t)j * words + w];
      });
}

template <int WORDS>
__device__ __forceinline__ uint32_t win_popc(const uint32_t (&qd)[WORDS], const uint32_t *__restrict__ e) {
  uint32_t t[WORDS];
  if constexpr (WORDS >= 4) {                           // entries are WORDS * 4 bytes apart from a 256-byte aligned base
#pragma unroll
    for (int k = 0; k < WORDS; k += 4) {
      const uint4 v = *(const uint4 *)(e + k);
      t[k] = v.x, t[k + 1] = v.y, t[k + 2] = v.z, t[k + 3] = v.w;
    }
  } else if constexpr (WORDS == 2) {
    const uint2 v = *(const uint2 *)e;
    t[0] = v.x, t[1] = v.y;
  } else {
    t[0] = e[0];
  }
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < WORDS; k++) d += (uint32_t)__popc(qd[k] ^ t[k]);
  return d;
}

// Clip-and-walk over one level's grid (L: a ScaledLevel, or a ScaledHit's fields of it): the window [x0, x1] x [y0, y1]
// clipped to the level's mapped extent [0, ext_x] x [0, ext_y] (its train entries all lie inside it), the cell rows
// that overlap it, and in each row's run of entries every WIN_LPQ-th one from lane `sub` on: visit(e, ent_meta[e]).
template <class Level, class Visit>
__device__ __forceinline__ void win_walk(const Level &L, const uint32_t *__restrict__ off_b,
                                         const uint2 *__restrict__ mp, uint32_t sub, int32_t x0, int32_t x1, int32_t y0,
                                         int32_t y1, Visit &&visit) {
  x0 = max(x0, 0), x1 = min(x1, L.ext_x);
  y0 = max(y0, 0), y1 = min(y1, L.ext_y);
  if (x0 > x1 || y0 > y1) return;
  const int32_t cx0 = x0 / L.side, cx1 = x1 / L.side, cy0 = y0 / L.side, cy1 = y1 / L.side;
  const uint32_t *off = off_b + L.base;
  for (int32_t cy = cy0; cy <= cy1; cy++) {
    const uint32_t e1 = off[cy * L.ncx + cx1 + 1];
    for (uint32_t e = off[cy * L.ncx + cx0] + sub; e < e1; e += WIN_LPQ) visit(e, mp[e]);
  }
}

constexpr int32_t SCALED_PRED_LIMIT = 1 << 20;   // predicted centres are clamped to [-2^20, 2^20]

// grid (query tiles, batch), WIN_THREADS threads; q_stride / t_stride in entries; qpred [batch][q_stride][2] or null;
// outputs [batch][q_stride].  ONE_LEVEL: the plan's span is 0.
template <int WORDS, bool ONE_LEVEL>
__global__ __launch_bounds__(WIN_THREADS) void k_match_scaled(ScaledPlan P, const uint32_t *__restrict__ qkp,
                                                              const uint32_t *__restrict__ qdesc,
                                                              const uint32_t *__restrict__ qcount,
                                                              const int32_t *__restrict__ qpred, size_t q_stride,
                                                              size_t t_stride, const uint32_t *__restrict__ cell_off,
                                                              const uint2 *__restrict__ ent_meta,
                                                              const uint32_t *__restrict__ ent_desc,
                                                              int32_t *__restrict__ idx, uint32_t *__restrict__ dist,
                                                              uint32_t *__restrict__ dist2) {
  const int b = blockIdx.y;
  const uint32_t nq = win_count(qcount[b], q_stride);
  const uint32_t sub = threadIdx.x % WIN_LPQ;
  const uint32_t *off_b = cell_off + (size_t)b * (P.ncells + 1);
  const uint2 *mp = ent_meta + (size_t)b * t_stride;
  const uint32_t *ep = ent_desc + (size_t)b * t_stride * WORDS;
  for (uint32_t q0 = blockIdx.x * (uint32_t)WIN_QPW; q0 < nq; q0 += gridDim.x * (uint32_t)WIN_QPW) {
    const uint32_t i = q0 + threadIdx.x / WIN_LPQ;
    const size_t o = (size_t)b * q_stride + i;
    uint32_t best = 0xffffffffu, second = 0xffffffffu;
    ScaledHit h{-1, 0, 0, 0, 0, 0, 0, 1, 0, 0};         // level -1: no candidates (past the count, or in no level)
    int32_t xc = 0, yc = 0;
    const uint32_t *qp = nullptr;
    if (i < nq) {
      const uint32_t k = qkp[o];
      const int32_t x = (int32_t)((k >> 12) & 0xfffu), y = (int32_t)(k & 0xfffu);
      h = sc_level(P, x, y);
      if (h.level >= 0) {
        if (qpred) {
          xc = min(max(qpred[o * 2], -SCALED_PRED_LIMIT), SCALED_PRED_LIMIT);
          yc = min(max(qpred[o * 2 + 1], -SCALED_PRED_LIMIT), SCALED_PRED_LIMIT);
        } else {
          xc = sc_map(x - h.col0, h.scale);
          yc = sc_map(y - h.row0, h.scale);
        }
        qp = qdesc + o * WORDS;
      }
    }
    uint32_t qd[WORDS];
    load_query<WORDS>(qd, qp);
    const int32_t r = h.radius;
    auto visit = [&](uint32_t e, uint2 m) {
      const int32_t tx = (int32_t)(m.x >> 16), ty = (int32_t)(m.x & 0xffffu);
      if (abs(tx - xc) <= r && abs(ty - yc) <= r)
        pair_push(best, second, (win_popc<WORDS>(qd, ep + (size_t)e * WORDS) << 16) | m.y);
    };
    if constexpr (ONE_LEVEL) {
      if (h.level >= 0) win_walk(h, off_b, mp, sub, xc - r, xc + r, yc - r, yc + r, visit);
    } else {
      for (int l = 0; l < P.nlevels; l++) {             // wave-uniform: the level's fields are kernel-argument loads
        if (h.level < 0 || abs(l - h.level) > P.span) continue;
        win_walk(P.lv[l], off_b, mp, sub, xc - r, xc + r, yc - r, yc + r, visit);
      }
    }
    pair_merge_lanes<WIN_LPQ>(best, second);
    if (sub == 0 && i < nq) store_match(o, best, second, idx, dist, dist2);
  }
}

// ---------------------------------------------------------------------------
// Rectified stereo matching (include/pislam_hip.h): left keypoint i (query) against the right
// keypoints (train) of the same pair inside a row band, then an SAD refinement on the pyramid images, a parabola fit
// and a per-pair median cut.  Four launches:
//   k_scaled_index    the right keypoints, with a ScaledPlan whose radius is row_radius0 and whose cell side comes from
//                     it (host: stereo_plan), unchanged from the scaled window matcher.
//   k_match_stereo    WIN_LPQ lanes per left keypoint; a wave-uniform loop over the plan's levels; the cell rows the
//                     band |Yl - Yr| <= row_radius0[lr] overlaps, columns Xl - max_disp .. Xl - min_disp, clipped to the
//                     level's mapped extent (win_walk); exact test, best on dist << 16 | j.  Writes idx / dist.
//   k_stereo_refine   ST_LPQ lanes per left keypoint (one patch row each): the 2L + 1 SADs of the (2w+1)^2 patch, the
//                     argmin, the parabola fit and the disparity.  w and L are kernel arguments, so the unrolled column
//                     and offset loops are cut by uniform branches and the register arrays are only indexed by
//                     compile-time constants.  Writes disp_q8 / sad.
//   k_stereo_median   one workgroup per pair: the n/2-th accepted SAD by a two-pass LDS radix select (SADs are below
//                     2^17: 8 high bits, then 9 low bits), the outlier cut and the count of accepted matches.
// ---------------------------------------------------------------------------
constexpr int ST_MAX_W = 7;            // sad_radius limit: patch rows / columns 2w + 1 <= 15
constexpr int ST_MAX_L = 8;            // search_radius limit: 2L + 1 <= 17 offsets
constexpr int ST_LPQ = 16;             // lanes per left keypoint in k_stereo_refine (>= 2 * ST_MAX_W + 1)
constexpr int ST_THREADS = 256;
constexpr int ST_QPW = ST_THREADS / ST_LPQ;
constexpr int ST_MEDIAN_THREADS = 1024;

// grid (query tiles, batch), WIN_THREADS threads; l_stride / r_stride in entries; outputs [batch][l_stride].
template <int WORDS>
__global__ __launch_bounds__(WIN_THREADS) void k_match_stereo(ScaledPlan P, int32_t min_disp, int32_t max_disp,
                                                              const uint32_t *__restrict__ lkp,
                                                              const uint32_t *__restrict__ ldesc,
                                                              const uint32_t *__restrict__ lcount, size_t l_stride,
                                                              size_t r_stride, const uint32_t *__restrict__ cell_off,
                                                              const uint2 *__restrict__ ent_meta,
                                                              const uint32_t *__restrict__ ent_desc,
                                                              int32_t *__restrict__ idx, uint32_t *__restrict__ dist) {
  const int b = blockIdx.y;
  const uint32_t nq = win_count(lcount[b], l_stride);
  const uint32_t sub = threadIdx.x % WIN_LPQ;
  const uint32_t *off_b = cell_off + (size_t)b * (P.ncells + 1);
  const uint2 *mp = ent_meta + (size_t)b * r_stride;
  const uint32_t *ep = ent_desc + (size_t)b * r_stride * WORDS;
  for (uint32_t q0 = blockIdx.x * (uint32_t)WIN_QPW; q0 < nq; q0 += gridDim.x * (uint32_t)WIN_QPW) {
    const uint32_t i = q0 + threadIdx.x / WIN_LPQ;
    const size_t o = (size_t)b * l_stride + i;
    uint32_t best = 0xffffffffu;
    int32_t lq = -1, xl = 0, yl = 0;                    // lq -1: no candidates (past the count, or in no level)
    const uint32_t *qp = nullptr;
    if (i < nq) {
      const uint32_t k = lkp[o];
      const int32_t x = (int32_t)((k >> 12) & 0xfffu), y = (int32_t)(k & 0xfffu);
      const ScaledHit h = sc_level(P, x, y);
      if (h.level >= 0) {
        lq = h.level;
        xl = sc_map(x - h.col0, h.scale);
        yl = sc_map(y - h.row0, h.scale);
        qp = ldesc + o * WORDS;
      }
    }
    uint32_t qd[WORDS];
    load_query<WORDS>(qd, qp);
    for (int l = 0; l < P.nlevels; l++) {               // wave-uniform: the level's fields are kernel-argument loads
      if (lq < 0 || abs(l - lq) > P.span) continue;
      const int32_t r = P.lv[l].radius;                 // row_radius0 of the RIGHT level
      win_walk(P.lv[l], off_b, mp, sub, xl - max_disp, xl - min_disp, yl - r, yl + r, [&](uint32_t e, uint2 m) {
        const int32_t dx = xl - (int32_t)(m.x >> 16), ty = (int32_t)(m.x & 0xffffu);
        if (abs(ty - yl) <= r && dx >= min_disp && dx <= max_disp)
          best = min(best, (win_popc<WORDS>(qd, ep + (size_t)e * WORDS) << 16) | m.y);
      });
    }
#pragma unroll
    for (int s = 1; s < WIN_LPQ; s <<= 1) best = min(best, __shfl_xor(best, s, 64));
    if (sub == 0 && i < nq) store_match(o, best, idx, dist);
  }
}

// The levels whose rectangles hold the left position (x, y) and the right position (xr, yr): the left level's
// rectangle and scale and the right position's mapped X, picked by selects in one wave-uniform loop.
struct StereoHit {
  int32_t col0, row0, width, height, scale, xr;
};
__device__ __forceinline__ StereoHit st_levels(const ScaledPlan &P, int32_t x, int32_t y, int32_t xr, int32_t yr) {
  StereoHit h{0, 0, 0, 0, 65536, 0};
  for (int l = 0; l < P.nlevels; l++) {
    const ScaledLevel L = P.lv[l];
    if ((uint32_t)(x - L.col0) < (uint32_t)L.width && (uint32_t)(y - L.row0) < (uint32_t)L.height)
      h.col0 = L.col0, h.row0 = L.row0, h.width = L.width, h.height = L.height, h.scale = L.scale;
    if ((uint32_t)(xr - L.col0) < (uint32_t)L.width && (uint32_t)(yr - L.row0) < (uint32_t)L.height)
      h.xr = sc_map(xr - L.col0, L.scale);
  }
  return h;
}

// floor(a / b) for b > 0
__device__ __forceinline__ int64_t st_floordiv(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// grid (query tiles, batch), ST_THREADS threads; pyramids uint8 [batch] at pyramid_stride bytes, rows of vstep bytes.
// Reads idx / dist of k_match_stereo and writes disp_q8 / sad for every left entry below the count.  W = sad_radius
// (a template argument: the patch columns need no branches); L = search_radius.
template <int W>
__global__ __launch_bounds__(ST_THREADS) void k_stereo_refine(ScaledPlan P, uint32_t max_hamming, int32_t L, int32_t min_disp, int32_t max_disp,
                                                              const uint8_t *__restrict__ lpyr,
                                                              const uint8_t *__restrict__ rpyr, int32_t vstep,
                                                              size_t pyramid_stride, const uint32_t *__restrict__ lkp,
                                                              const uint32_t *__restrict__ lcount, size_t l_stride,
                                                              const uint32_t *__restrict__ rkp, size_t r_stride,
                                                              const int32_t *__restrict__ idx,
                                                              const uint32_t *__restrict__ dist,
                                                              int32_t *__restrict__ disp_q8, uint32_t *__restrict__ sad) {
  constexpr int32_t w = W;
  const int b = blockIdx.y;
  const uint32_t nq = win_count(lcount[b], l_stride);
  const int32_t sub = (int32_t)(threadIdx.x % ST_LPQ);
  const uint8_t *lp = lpyr + (size_t)b * pyramid_stride, *rp = rpyr + (size_t)b * pyramid_stride;
  for (uint32_t q0 = blockIdx.x * (uint32_t)ST_QPW; q0 < nq; q0 += gridDim.x * (uint32_t)ST_QPW) {
    const uint32_t i = q0 + threadIdx.x / ST_LPQ;
    const size_t o = (size_t)b * l_stride + i;
    bool ok = false;
    int32_t ul = 0, vl = 0, scale = 65536;
    int64_t ur0 = 0;
    const uint8_t *lrow = lp, *rrow = rp;               // level ll's row vl: column col0 + ul (left), col0 + ur0 (right)
    if (i < nq && dist[o] <= max_hamming) {
      const uint32_t kl = lkp[o], kr = rkp[(size_t)b * r_stride + (uint32_t)idx[o]];
      // (a match has both positions in a level: k_match_stereo and k_scaled_index skip the others)
      const StereoHit hl = st_levels(P, (int32_t)((kl >> 12) & 0xfffu), (int32_t)(kl & 0xfffu),
                                     (int32_t)((kr >> 12) & 0xfffu), (int32_t)(kr & 0xfffu));
      ul = (int32_t)((kl >> 12) & 0xfffu) - hl.col0;
      vl = (int32_t)(kl & 0xfffu) - hl.row0;
      scale = hl.scale;
      ur0 = ((int64_t)hl.xr * 65536 + scale / 2) / scale;
      // every pixel of every offset's patch inside level ll's rectangle
      ok = ul - w >= 0 && ul + w < hl.width && vl - w >= 0 && vl + w < hl.height && ur0 - L - w >= 0 &&
           ur0 + L + w < hl.width;
      const size_t row = (size_t)(hl.row0 + vl) * vstep + hl.col0;
      lrow = lp + row + ul;
      rrow = rp + row + (ok ? ur0 : 0);
    }
    // this lane's patch row dy = sub - w (lanes past 2w + 1 add nothing)
    uint32_t s[2 * ST_MAX_L + 1];
#pragma unroll
    for (int t = 0; t < 2 * ST_MAX_L + 1; t++) s[t] = 0;
    if (ok && sub <= 2 * w) {
      const int32_t dy = sub - w;
      const int32_t cl = lrow[0];
      const uint8_t *la = lrow + (ptrdiff_t)dy * vstep - w, *ra = rrow + (ptrdiff_t)dy * vstep - L - w;
      // all ST_MAX_L offsets on either side, the reads clamped to the 2L + 1 in range (no branches on L: the offsets
      // past L are computed from repeated pixels and never looked at)
      // (the clamps are kept in vector registers: as scalars the compiler hoists all of them and spills)
      uint32_t lim_r = 2 * (W + L), lim_c = 2 * L;
      asm("" : "+v"(lim_r), "+v"(lim_c));
      const uint8_t *ca = rrow - L;
      int32_t a[2 * W + 1], rv[2 * W + 2 * ST_MAX_L + 1], cr[2 * ST_MAX_L + 1];
#pragma unroll
      for (int k = 0; k < 2 * W + 1; k++) a[k] = (int32_t)la[k] - cl;
#pragma unroll
      for (int k = 0; k < 2 * W + 2 * ST_MAX_L + 1; k++) rv[k] = ra[min((uint32_t)k, lim_r)];
#pragma unroll
      for (int t = 0; t < 2 * ST_MAX_L + 1; t++) cr[t] = ca[min((uint32_t)t, lim_c)];
#pragma unroll
      for (int t = 0; t < 2 * ST_MAX_L + 1; t++) {
#pragma unroll
        for (int k = 0; k < 2 * W + 1; k++) s[t] += (uint32_t)abs(a[k] - (rv[k + t] - cr[t]));
      }
    }
#pragma unroll
    for (int t = 0; t < 2 * ST_MAX_L + 1; t++) {
#pragma unroll
      for (int d = 1; d < ST_LPQ; d <<= 1) s[t] += __shfl_xor(s[t], d, 64);
    }
    if (sub == 0 && i < nq) {
      int32_t out_disp = -1;
      uint32_t out_sad = 0xffffffffu;
      if (ok) {
        // argmin (ties: the smallest offset), then its neighbours, by compile-time indexing only
        uint32_t d2 = s[0];
        int32_t tb = 0;
#pragma unroll
        for (int t = 1; t < 2 * ST_MAX_L + 1; t++)
          if (s[t] < d2 && t <= 2 * L) d2 = s[t], tb = t;
        if (tb != 0 && tb != 2 * L) {
          uint32_t d1 = 0, d3 = 0;
#pragma unroll
          for (int t = 0; t < 2 * ST_MAX_L + 1; t++) {
            if (t == tb - 1) d1 = s[t];
            if (t == tb + 1) d3 = s[t];
          }
          const int64_t num = (int64_t)d1 - d3, den = 2 * ((int64_t)d1 + d3 - 2 * (int64_t)d2);
          const int64_t delta = den == 0 ? 0 : st_floordiv(512 * num + den, 2 * den);
          const int64_t dl = 256 * ((int64_t)ul - ur0 - (tb - L)) - delta;
          const int64_t disp = (dl * scale + 32768) >> 16;        // arithmetic shift: floor
          if (disp >= 256 * (int64_t)min_disp && disp <= 256 * (int64_t)max_disp) {
            out_disp = (int32_t)max(disp, (int64_t)1);
            out_sad = d2;
          }
        }
      }
      disp_q8[o] = out_disp;
      sad[o] = out_sad;
    }
  }
}

// Wave 0 of the workgroup: the bin of hist[0 .. NB) that holds rank k (cumulative counts), and the rank inside it.
template <int NB>
__device__ __forceinline__ void st_select_bin(const uint32_t *hist, uint32_t k, uint32_t *bin, uint32_t *rank) {
  constexpr int PER = NB / 64;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t c[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) sum += (c[j] = hist[lane * PER + j]);
  uint32_t incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(incl, d, 64);
    if ((int)lane >= d) incl += v;
  }
  uint32_t run = incl - sum;
  // the one lane whose range [run, incl) holds k
  if (k >= run && k < incl) {
#pragma unroll
    for (int j = 0; j < PER; j++) {
      if (k >= run && k < run + c[j]) *bin = lane * PER + j, *rank = k - run;
      run += c[j];
    }
  }
}

// grid (batch), ST_MEDIAN_THREADS threads.  median_filter 0: only counts (nstereo must then be non-null).
__global__ __launch_bounds__(ST_MEDIAN_THREADS) void k_stereo_median(int32_t median_filter,
                                                                     const uint32_t *__restrict__ lcount, size_t l_stride,
                                                                     int32_t *__restrict__ disp_q8,
                                                                     uint32_t *__restrict__ sad,
                                                                     uint32_t *__restrict__ nstereo) {
  __shared__ uint32_t hist[512];
  __shared__ uint32_t sel[3];                            // accepted count, high bin, rank inside it / low bin
  const int b = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t nq = win_count(lcount[b], l_stride);
  int32_t *dp = disp_q8 + (size_t)b * l_stride;
  uint32_t *sp = sad + (size_t)b * l_stride;
  for (uint32_t c = tid; c < 512; c += ST_MEDIAN_THREADS) hist[c] = 0;
  if (tid == 0) sel[0] = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t i = tid; i < nq; i += ST_MEDIAN_THREADS) {
    const uint32_t v = sp[i];
    if (v == 0xffffffffu) continue;
    mine++;
    if (median_filter) atomicAdd(&hist[v >> 9], 1u);   // SADs are at most 225 * 510 < 2^17: 256 high bins
  }
  if (mine) atomicAdd(&sel[0], mine);
  __syncthreads();
  const uint32_t n = sel[0];
  if (!median_filter || n == 0) {
    if (tid == 0 && nstereo) nstereo[b] = n;
    return;
  }
  if (tid < 64) st_select_bin<256>(hist, n / 2, &sel[1], &sel[2]);
  __syncthreads();
  const uint32_t hi = sel[1], k = sel[2];
  for (uint32_t c = tid; c < 512; c += ST_MEDIAN_THREADS) hist[c] = 0;
  __syncthreads();
  for (uint32_t i = tid; i < nq; i += ST_MEDIAN_THREADS) {
    const uint32_t v = sp[i];
    if (v != 0xffffffffu && (v >> 9) == hi) atomicAdd(&hist[v & 511u], 1u);
  }
  __syncthreads();
  if (tid < 64) st_select_bin<512>(hist, k, &sel[2], &sel[1]);
  __syncthreads();
  const uint32_t m = hi << 9 | sel[2];
  if (tid == 0) sel[0] = 0;
  __syncthreads();
  // outliers: 10 * sad > 21 * m (sad > 1.5 * 1.4 * m), kept: counted
  uint32_t kept = 0;
  for (uint32_t i = tid; i < nq; i += ST_MEDIAN_THREADS) {
    const uint32_t v = sp[i];
    if (v == 0xffffffffu) continue;
    if (10u * v > 21u * m) {
      dp[i] = -1;
      sp[i] = 0xffffffffu;
    } else {
      kept++;
    }
  }
  if (kept) atomicAdd(&sel[0], kept);
  __syncthreads();
  if (tid == 0 && nstereo) nstereo[b] = sel[0];
}


}  // namespace pm
