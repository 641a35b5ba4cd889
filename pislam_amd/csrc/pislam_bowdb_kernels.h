// Key-frame database for bag-of-words place recognition (include/pislam_hip.h): integer tf-idf
// weights, an inverted file over the words of the stored key frames, and a query that scores every key frame against a
// bag-of-words vector and selects the best k.  All arithmetic is integer, all accumulation is integer addition or
// maximum, so no result depends on the order in which atomics arrive.  The reference ships nothing of the kind: the
// semantics are this library's own.
//   k_bow_weight      one workgroup per frame: A = sum tf * idf in 64 bits, then (a_k << 24) / A per entry.
//   k_db_store        one workgroup per added frame: the entries go to the forward store, the words' counts (global
//                     memory, integer atomics) grow by the new entries.
//   k_db_scan_*       exclusive scan of the counts into the CSR offsets (pm::block_scan in each): chunk sums, one
//                     workgroup over the chunk sums, offsets and scatter cursors per chunk.
//   k_db_scatter      one workgroup per stored frame: every entry takes the next free slot of its word.  Posting order
//                     inside a word varies between runs; no result does.
//   k_db_accumulate   one workgroup per (slice of ids, query).  The (score, common) cells of the slice live in LDS: a
//                     32-bit score plane and a 16-bit common plane (two ids per dword: common <= 16384 never carries).
//                     DB_LPW lanes walk the posting list of one query word; lists longer than DB_LONG are queued and walked
//                     by the whole workgroup afterwards, so one stop word does not serialise on 16 lanes.  The planes
//                     are then stored to the workspace (coalesced) and the slice's largest eligible `common` goes into
//                     the query's maximum with one integer atomicMax per workgroup.
//   k_db_select       one workgroup per (DB_SEL_SLICE ids, query): candidates by the now known maximum, keys
//                     score << 32 | ~id in registers (DB_SEL_R per thread), the largest taken topk times.  With one
//                     slice it writes the results, else a partial list.
//   k_db_merge        one workgroup per query: the same extraction over the partial lists (at most 128 * 64 keys).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pislam_match_kernels.h"

namespace pd {

constexpr int DB_THREADS = 1024;
constexpr int DB_WAVES = DB_THREADS / 64;
constexpr int DB_MAX_STRIDE = 16384;                  // entries of a bag-of-words vector (pb::BOW_VEC_MAX)
constexpr int DB_MAX_TOPK = 64;
constexpr int DB_MAX_CAPACITY = 1 << 20;
constexpr int DB_SCAN_PER_THREAD = 16;
constexpr int DB_SCAN_CHUNK = DB_THREADS * DB_SCAN_PER_THREAD;   // 2^24 words: at most 1024 chunks, one thread each
constexpr int DB_STORE_THREADS = 256;
constexpr int DB_ACC_MAX_SLICE = 24576;               // ids per accumulate workgroup: 6 bytes each = 144 KiB of LDS
constexpr int DB_LPW = 16;                            // lanes per query word
constexpr int DB_LONG = 1024;                         // longer posting lists are walked by the whole workgroup
constexpr int DB_QUEUE = 2048;                        // such lists per query that can be deferred (more: walked in place)
constexpr int DB_SEL_R = 8;                           // keys per thread
constexpr int DB_SEL_SLICE = DB_THREADS * DB_SEL_R;   // 8192 ids; 2^20 / 8192 * 64 = 8192 partial keys at most

__device__ __forceinline__ uint64_t db_shfl_xor64(uint64_t v, int s) {
  const uint32_t lo = __shfl_xor((uint32_t)v, s, 64), hi = __shfl_xor((uint32_t)(v >> 32), s, 64);
  return ((uint64_t)hi << 32) | lo;
}

// grid (batch), DB_THREADS threads.  Layouts [batch][stride]; idf [nwords] or null (= 1 for every word).
__global__ __launch_bounds__(DB_THREADS) void k_bow_weight(const uint32_t *__restrict__ bow_word,
                                                           const uint32_t *__restrict__ bow_tf,
                                                           const uint32_t *__restrict__ bow_n, size_t stride,
                                                           const uint32_t *__restrict__ idf, uint32_t nwords,
                                                           uint32_t *__restrict__ bow_weight) {
  __shared__ uint64_t wave_sum[DB_WAVES];
  const int b = blockIdx.x;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = pm::win_count(bow_n[b], stride);
  const uint32_t *wp = bow_word + (size_t)b * stride, *tp = bow_tf + (size_t)b * stride;
  auto a_of = [&](uint32_t k) -> uint64_t {
    const uint32_t w = wp[k];
    if (w >= nwords) return 0;
    return (uint64_t)tp[k] * (idf ? min(idf[w], 65535u) : 1u);
  };
  uint64_t s = 0;
  for (uint32_t k = tid; k < n; k += DB_THREADS) s += a_of(k);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += db_shfl_xor64(s, d);
  if (lane == 0) wave_sum[wave] = s;
  __syncthreads();
  uint64_t A = 0;
  for (int w = 0; w < DB_WAVES; w++) A += wave_sum[w];
  uint32_t *op = bow_weight + (size_t)b * stride;
  for (uint32_t k = tid; k < n; k += DB_THREADS) op[k] = A == 0 ? 0u : (uint32_t)((a_of(k) << 24) / A);
}

// grid (frames added), DB_STORE_THREADS threads.  Frame b becomes key frame first_id + b: its first
// min(bow_n[b], stride, db_stride) entries go to fwd_word / fwd_weight [capacity][db_stride], cnt[word] grows.
__global__ __launch_bounds__(DB_STORE_THREADS) void k_db_store(uint32_t first_id, uint32_t db_stride, uint32_t nwords,
                                                               const uint32_t *__restrict__ bow_word,
                                                               const uint32_t *__restrict__ bow_weight,
                                                               const uint32_t *__restrict__ bow_n, size_t stride,
                                                               uint32_t *__restrict__ fwd_word,
                                                               uint32_t *__restrict__ fwd_weight,
                                                               uint32_t *__restrict__ fwd_n, uint8_t *__restrict__ alive,
                                                               uint32_t *__restrict__ cnt, uint32_t *__restrict__ dev_size) {
  const uint32_t b = blockIdx.x, id = first_id + b;
  const uint32_t n = min(pm::win_count(bow_n[b], stride), db_stride);
  const uint32_t *wp = bow_word + (size_t)b * stride, *vp = bow_weight + (size_t)b * stride;
  uint32_t *ow = fwd_word + (size_t)id * db_stride, *ov = fwd_weight + (size_t)id * db_stride;
  for (uint32_t j = threadIdx.x; j < n; j += DB_STORE_THREADS) {
    const uint32_t w = wp[j];
    ow[j] = w;
    ov[j] = vp[j];
    if (w < nwords) atomicAdd(&cnt[w], 1u);
  }
  if (threadIdx.x == 0) {
    fwd_n[id] = n;
    alive[id] = 1;
    if (b == 0) *dev_size = first_id + gridDim.x;
  }
}

__device__ __forceinline__ uint32_t db_chunk_sum(const uint32_t *__restrict__ cnt, uint32_t nwords, uint32_t i0) {
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < DB_SCAN_PER_THREAD; k++) s += i0 + k < nwords ? cnt[i0 + k] : 0u;
  return s;
}

// grid (chunks of DB_SCAN_CHUNK words), DB_THREADS threads: bsum[chunk] = the chunk's entries.
__global__ __launch_bounds__(DB_THREADS) void k_db_scan_chunks(const uint32_t *__restrict__ cnt, uint32_t nwords,
                                                               uint32_t *__restrict__ bsum) {
  __shared__ uint32_t wave_sum[DB_WAVES];
  const uint32_t i0 = blockIdx.x * (uint32_t)DB_SCAN_CHUNK + threadIdx.x * (uint32_t)DB_SCAN_PER_THREAD;
  uint32_t total;
  (void)pm::block_scan<DB_THREADS>(db_chunk_sum(cnt, nwords, i0), wave_sum, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum becomes its own exclusive scan (nchunks <= DB_THREADS), word_off[nwords] = all entries.
__global__ __launch_bounds__(DB_THREADS) void k_db_scan_sums(uint32_t nchunks, uint32_t nwords, uint32_t *__restrict__ bsum,
                                                             uint32_t *__restrict__ word_off) {
  __shared__ uint32_t wave_sum[DB_WAVES];
  uint32_t total;
  const uint32_t run = pm::block_scan<DB_THREADS>(threadIdx.x < nchunks ? bsum[threadIdx.x] : 0u, wave_sum, &total);
  if (threadIdx.x < nchunks) bsum[threadIdx.x] = run;
  if (threadIdx.x == 0) word_off[nwords] = total;
}

// grid (chunks): word_off[w] = cursor[w] = entries of the words below w.
__global__ __launch_bounds__(DB_THREADS) void k_db_scan_offsets(const uint32_t *__restrict__ cnt, uint32_t nwords,
                                                                const uint32_t *__restrict__ bsum,
                                                                uint32_t *__restrict__ word_off,
                                                                uint32_t *__restrict__ cursor) {
  __shared__ uint32_t wave_sum[DB_WAVES];
  const uint32_t i0 = blockIdx.x * (uint32_t)DB_SCAN_CHUNK + threadIdx.x * (uint32_t)DB_SCAN_PER_THREAD;
  uint32_t total;
  uint32_t run = pm::block_scan<DB_THREADS>(db_chunk_sum(cnt, nwords, i0), wave_sum, &total) + bsum[blockIdx.x];
  for (int k = 0; k < DB_SCAN_PER_THREAD; k++) {
    const uint32_t i = i0 + k;
    if (i >= nwords) break;
    word_off[i] = run;
    cursor[i] = run;
    run += cnt[i];
  }
}

// grid (key frames stored), DB_STORE_THREADS threads: post[slot] = (id, weight), slot = the next free one of the word.
// cnt counted exactly the entries stored, so every slot lies below word_off[nwords] <= capacity * db_stride.
__global__ __launch_bounds__(DB_STORE_THREADS) void k_db_scatter(uint32_t db_stride, uint32_t nwords,
                                                                 const uint32_t *__restrict__ fwd_word,
                                                                 const uint32_t *__restrict__ fwd_weight,
                                                                 const uint32_t *__restrict__ fwd_n,
                                                                 uint32_t *__restrict__ cursor, uint2 *__restrict__ post) {
  const uint32_t id = blockIdx.x;
  const uint32_t n = min(fwd_n[id], db_stride);
  const uint32_t *wp = fwd_word + (size_t)id * db_stride, *vp = fwd_weight + (size_t)id * db_stride;
  for (uint32_t j = threadIdx.x; j < n; j += DB_STORE_THREADS) {
    const uint32_t w = wp[j];
    if (w >= nwords) continue;
    const uint32_t slot = atomicAdd(&cursor[w], 1u);
    post[slot] = make_uint2(id, vp[j]);
  }
}

// grid (slices, batch), DB_THREADS threads, dynamic LDS 6 * slice bytes (slice even).  Slices are laid over the
// CAPACITY and cut at the number of key frames the device holds now (*dev_size), so a captured launch serves a database
// that has grown since.  acc_score [batch][cap_pad] uint32, acc_common [batch][cap_pad] uint16 (cap_pad even), written
// for the ids below *dev_size; gmax [batch] was zeroed before the launch.
__global__ __launch_bounds__(DB_THREADS) void k_db_accumulate(uint32_t nwords, uint32_t cap_pad, uint32_t slice,
                                                              const uint32_t *__restrict__ dev_size,
                                                              const uint8_t *__restrict__ alive,
                                                              const uint32_t *__restrict__ word_off,
                                                              const uint2 *__restrict__ post,
                                                              const uint32_t *__restrict__ q_word,
                                                              const uint32_t *__restrict__ q_weight,
                                                              const uint32_t *__restrict__ q_n, size_t stride,
                                                              const int32_t *__restrict__ id_limit,
                                                              uint32_t *__restrict__ acc_score,
                                                              uint32_t *__restrict__ acc_common,
                                                              uint32_t *__restrict__ gmax) {
  extern __shared__ uint32_t db_lds[];                   // score [slice], common [slice / 2] (two ids per dword)
  __shared__ uint16_t queue[DB_QUEUE];
  __shared__ uint32_t queued;
  __shared__ uint32_t wave_max[DB_WAVES];
  const uint32_t b = blockIdx.y, s0 = blockIdx.x * slice, size = *dev_size;
  if (s0 >= size) return;                                // (workgroup-uniform)
  const uint32_t ns = min(slice, size - s0);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t *sc = db_lds, *cm = db_lds + slice;
  for (uint32_t l = tid; l < slice + slice / 2; l += DB_THREADS) db_lds[l] = 0;
  if (tid == 0) queued = 0;
  __syncthreads();
  auto add = [&](uint2 p, uint32_t v) {
    const uint32_t l = p.x - s0;                         // (an id below the slice wraps to a large number)
    if (l < ns) {
      atomicAdd(&sc[l], min(v, p.y));
      atomicAdd(&cm[l >> 1], 1u << ((l & 1u) * 16));
    }
  };
  const uint32_t n = pm::win_count(q_n[b], stride);
  const uint32_t *qw = q_word + (size_t)b * stride, *qv = q_weight + (size_t)b * stride;
  const uint32_t sub = tid % DB_LPW, grp = tid / DB_LPW;
  for (uint32_t i0 = 0; i0 < n; i0 += DB_THREADS / DB_LPW) {
    const uint32_t i = i0 + grp;
    uint32_t e = 0, e1 = 0, v = 0;
    if (i < n) {
      const uint32_t w = qw[i];
      if (w < nwords) e = word_off[w], e1 = word_off[w + 1], v = qv[i];
    }
    // a long list is handed to the whole workgroup (every lane takes part in the shuffle: the loop is uniform)
    const bool is_long = e1 - e > (uint32_t)DB_LONG;
    uint32_t slot = DB_QUEUE;
    if (is_long && sub == 0) slot = atomicAdd(&queued, 1u);
    slot = __shfl(slot, (int)(lane & ~(uint32_t)(DB_LPW - 1)), 64);
    if (is_long && slot < (uint32_t)DB_QUEUE) {
      if (sub == 0) queue[slot] = (uint16_t)i;           // (i < DB_MAX_STRIDE)
      e1 = e;
    }
    for (e += sub; e < e1; e += DB_LPW) add(post[e], v);
  }
  __syncthreads();
  const uint32_t nq = min(queued, (uint32_t)DB_QUEUE);
  for (uint32_t k = 0; k < nq; k++) {
    const uint32_t i = queue[k], w = qw[i], v = qv[i];
    for (uint32_t e = word_off[w] + tid, e1 = word_off[w + 1]; e < e1; e += DB_THREADS) add(post[e], v);
  }
  __syncthreads();
  const int32_t lim = id_limit ? id_limit[b] : 0x7fffffff;
  uint32_t *os = acc_score + (size_t)b * cap_pad + s0;
  uint32_t *oc = acc_common + ((size_t)b * cap_pad + s0) / 2;   // (cap_pad and s0 are even)
  uint32_t m = 0;
  for (uint32_t l = tid; l < ns; l += DB_THREADS) {
    os[l] = sc[l];
    const uint32_t id = s0 + l, c = (cm[l >> 1] >> ((l & 1u) * 16)) & 0xffffu;
    if (alive[id] && (int32_t)id < lim) m = max(m, c);
  }
  for (uint32_t l = tid; l < (ns + 1) / 2; l += DB_THREADS) oc[l] = cm[l];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_xor(m, d, 64));
  if (lane == 0) wave_max[wave] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < DB_WAVES; w++) m = max(m, wave_max[w]);
    if (m) atomicMax(&gmax[b], m);
  }
}

// Takes the workgroup's largest non-zero key (they are distinct) `topk` times: emit(k, r) runs in the thread that holds
// it as key[r]; none(k) for the ranks left over.  wave_max: LDS [2][DB_WAVES], one barrier per round.
template <class Emit, class None>
__device__ __forceinline__ void db_extract(uint64_t (&key)[DB_SEL_R], int topk, uint64_t *wave_max, Emit emit, None none) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  int k = 0;
  for (; k < topk; k++) {
    uint64_t m = key[0];
#pragma unroll
    for (int r = 1; r < DB_SEL_R; r++) m = max(m, key[r]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, db_shfl_xor64(m, d));
    uint64_t *wm = wave_max + (k & 1) * DB_WAVES;
    if (lane == 0) wm[wave] = m;
    __syncthreads();
    uint64_t g = 0;
    for (int w = 0; w < DB_WAVES; w++) g = max(g, wm[w]);
    if (g == 0) break;                                   // (workgroup-uniform)
#pragma unroll
    for (int r = 0; r < DB_SEL_R; r++)
      if (key[r] == g) {
        emit(k, r, g);
        key[r] = 0;
      }
  }
  for (int j = k + (int)threadIdx.x; j < topk; j += DB_THREADS) none(j);
}

// grid (nsel, batch), DB_THREADS threads.  nsel == 1: writes top_* [batch][topk] and max_common; else the partial
// lists pkey / pcom [batch][nsel][topk] (key 0 = no candidate).
__global__ __launch_bounds__(DB_THREADS) void k_db_select(uint32_t cap_pad, const uint32_t *__restrict__ dev_size,
                                                          const uint8_t *__restrict__ alive,
                                                          const int32_t *__restrict__ id_limit, uint32_t pct, int topk,
                                                          const uint32_t *__restrict__ acc_score,
                                                          const uint16_t *__restrict__ acc_common,
                                                          const uint32_t *__restrict__ gmax, uint64_t *__restrict__ pkey,
                                                          uint32_t *__restrict__ pcom, int32_t *__restrict__ top_id,
                                                          uint32_t *__restrict__ top_score,
                                                          uint32_t *__restrict__ top_common,
                                                          uint32_t *__restrict__ max_common) {
  __shared__ uint64_t wave_max[2 * DB_WAVES];
  const uint32_t b = blockIdx.y, sel = blockIdx.x, nsel = gridDim.x, size = *dev_size, gm = gmax[b];
  const int32_t lim = id_limit ? id_limit[b] : 0x7fffffff;
  uint64_t key[DB_SEL_R];
  uint32_t com[DB_SEL_R];
#pragma unroll
  for (int r = 0; r < DB_SEL_R; r++) {
    const uint32_t id = sel * (uint32_t)DB_SEL_SLICE + r * (uint32_t)DB_THREADS + threadIdx.x;
    key[r] = 0, com[r] = 0;
    if (id < size && alive[id] && (int32_t)id < lim) {
      const uint32_t c = acc_common[(size_t)b * cap_pad + id];
      if (c >= 1 && c * 100u >= pct * gm) {
        key[r] = ((uint64_t)acc_score[(size_t)b * cap_pad + id] << 32) | (uint32_t)~id;
        com[r] = c;
      }
    }
  }
  if (nsel == 1) {
    const size_t o = (size_t)b * topk;
    db_extract(
        key, topk, wave_max,
        [&](int k, int r, uint64_t g) {
          top_id[o + k] = (int32_t)~(uint32_t)g;
          top_score[o + k] = (uint32_t)(g >> 32);
          top_common[o + k] = com[r];
        },
        [&](int k) { top_id[o + k] = -1, top_score[o + k] = 0, top_common[o + k] = 0; });
    if (threadIdx.x == 0) max_common[b] = gm;
  } else {
    const size_t o = ((size_t)b * nsel + sel) * topk;
    db_extract(
        key, topk, wave_max, [&](int k, int r, uint64_t g) { pkey[o + k] = g, pcom[o + k] = com[r]; },
        [&](int k) { pkey[o + k] = 0, pcom[o + k] = 0; });
  }
}

// grid (batch), DB_THREADS threads: the best topk of the nsel * topk <= DB_SEL_SLICE partial keys of a query.
__global__ __launch_bounds__(DB_THREADS) void k_db_merge(uint32_t nsel, int topk, const uint64_t *__restrict__ pkey,
                                                         const uint32_t *__restrict__ pcom,
                                                         const uint32_t *__restrict__ gmax, int32_t *__restrict__ top_id,
                                                         uint32_t *__restrict__ top_score,
                                                         uint32_t *__restrict__ top_common,
                                                         uint32_t *__restrict__ max_common) {
  __shared__ uint64_t wave_max[2 * DB_WAVES];
  const uint32_t b = blockIdx.x, total = nsel * (uint32_t)topk;
  const uint64_t *kp = pkey + (size_t)b * total;
  const uint32_t *cp = pcom + (size_t)b * total;
  uint64_t key[DB_SEL_R];
#pragma unroll
  for (int r = 0; r < DB_SEL_R; r++) {
    const uint32_t i = r * (uint32_t)DB_THREADS + threadIdx.x;
    key[r] = i < total ? kp[i] : 0;
  }
  const size_t o = (size_t)b * topk;
  db_extract(
      key, topk, wave_max,
      [&](int k, int r, uint64_t g) {
        top_id[o + k] = (int32_t)~(uint32_t)g;
        top_score[o + k] = (uint32_t)(g >> 32);
        top_common[o + k] = cp[r * (uint32_t)DB_THREADS + threadIdx.x];
      },
      [&](int k) { top_id[o + k] = -1, top_score[o + k] = 0, top_common[o + k] = 0; });
  if (threadIdx.x == 0) max_common[b] = gmax[b];
}

}  // namespace pd
