// grapehip — MI355X (gfx950) GPU engine: kernels + host drivers.
//
// Hand-written CDNA4 HIP throughout (wave64, LDS-staged owner search, no
// Thrust/CUB/hipCUB). Reference parity map:
//   * cuda/parallel/parallel_engine.h LB schedulers -> expand_cm_* kernels
//     (LDS prefix owner-search; CTA/STRICT variants arrive in later rounds)
//   * cuda/utils/cuda_utils.h CUB scans -> hand-rolled hierarchical
//     exclusive scan (wave shfl scan + LDS cross-wave + recursive spine)
//   * cuda/parallel/gpu_message_manager.h -> HaloBuffer (global-vid dedup
//     bitmap + per-peer regions) exchanged with paired ncclSend/Recv over
//     xGMI, lengths via the TCP control plane
//   * cuda apps bfs/sssp/pagerank/wcc -> drivers below
//   * examples/analytical_apps/kcore/kcore.h and core_decomposition/
//     core_decomposition.h (CPU only in the reference) -> frontier peeling
//   * examples/analytical_apps/bc/staged_bc{,_bfs}.h (CPU only in the
//     reference) -> push BFS with path counts + level-queue replay
#include "gpu_engine.hpp"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <climits>
#include <cstring>
#include <type_traits>
#include <unordered_map>

#include "dev_graph.hpp"

#define NCCL_CHECK(expr)                                                   \
  do {                                                                     \
    ncclResult_t _r = (expr);                                              \
    if (_r != ncclSuccess) {                                               \
      throw std::runtime_error(std::string("RCCL error: ") +               \
                               ncclGetErrorString(_r));                    \
    }                                                                      \
  } while (0)

namespace grapehip {

// ===========================================================================
// Device utilities
// ===========================================================================

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

// atomicMin on non-negative float via ordered int reinterpret.
__device__ __forceinline__ float atomicMinPosFloat(float* addr, float val) {
  int old = atomicMin(reinterpret_cast<int*>(addr), __float_as_int(val));
  return __int_as_float(old);
}

// wave-inclusive scan (u64), 64 lanes
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint64_t up = __shfl_up(static_cast<unsigned long long>(v), d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// ===========================================================================
// Hierarchical exclusive scan: in (u32 or u64) -> out u64, returns total.
// Pass A: per-block sums; spine scanned recursively; pass B: final scan.
// ITEMS per thread keeps the spine small (405M rows -> ~200k blocks).
// ===========================================================================

constexpr int kScanItems = 8;
constexpr int kScanChunk = kBlock * kScanItems;  // 2048 elements per block

template <typename IN>
__global__ void scan_pass_a(const IN* __restrict__ in, size_t n,
                            uint64_t* __restrict__ bsums) {
  __shared__ uint64_t s_wave[kBlock / kWave];
  size_t base = static_cast<size_t>(blockIdx.x) * kScanChunk +
                static_cast<size_t>(threadIdx.x) * kScanItems;
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    size_t i = base + k;
    if (i < n) sum += in[i];
  }
  // wave reduce
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
    sum += __shfl_down(static_cast<unsigned long long>(sum), d, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) t += s_wave[w];
    bsums[blockIdx.x] = t;
  }
}

template <typename IN>
__global__ void scan_pass_b(const IN* __restrict__ in, size_t n,
                            const uint64_t* __restrict__ boffs,
                            uint64_t* __restrict__ out) {
  __shared__ uint64_t s_wave[kBlock / kWave];
  size_t base = static_cast<size_t>(blockIdx.x) * kScanChunk +
                static_cast<size_t>(threadIdx.x) * kScanItems;
  uint64_t vals[kScanItems];
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    size_t i = base + k;
    uint64_t v = i < n ? static_cast<uint64_t>(in[i]) : 0;
    vals[k] = sum;  // exclusive within thread
    sum += v;
  }
  uint64_t incl = wave_incl_scan(sum);
  uint64_t wave_excl = incl - sum;
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint64_t wave_base = 0;
  for (int w = 0; w < static_cast<int>(threadIdx.x >> 6); ++w)
    wave_base += s_wave[w];
  uint64_t thread_base = boffs[blockIdx.x] + wave_base + wave_excl;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    size_t i = base + k;
    if (i < n) out[i] = thread_base + vals[k];
  }
}

// Grow-only per-level scratch so per-round frontier scans never hipMalloc.
// Levels are FIXED-depth (2048^4 > 2^44 elements) so references returned by
// sum_buf/off_buf stay valid while deeper recursion levels allocate.
struct ScanTemp {
  static constexpr size_t kMaxLevels = 4;
  DeviceBuffer<uint64_t> sums[kMaxLevels];   // per level: block sums
  DeviceBuffer<uint64_t> offs[kMaxLevels];   // per level: scanned sums
  DeviceBuffer<uint64_t> zero;               // single 0 (spine base)
  DeviceBuffer<uint64_t>& sum_buf(size_t l, size_t n) {
    if (sums[l].size() < n) sums[l].resize(n + (n >> 2) + 16);
    return sums[l];
  }
  DeviceBuffer<uint64_t>& off_buf(size_t l, size_t n) {
    if (offs[l].size() < n) offs[l].resize(n + (n >> 2) + 16);
    return offs[l];
  }
};

template <typename IN>
void scan_recurse(const IN* d_in, uint64_t* d_out, size_t n, hipStream_t s,
                  ScanTemp& tmp, size_t level) {
  size_t nblocks = (n + kScanChunk - 1) / kScanChunk;
  if (nblocks <= 1) {
    if (tmp.zero.size() == 0) {
      tmp.zero.resize(1);
      tmp.zero.zero(s);
    }
    hipLaunchKernelGGL(scan_pass_b<IN>, dim3(1), dim3(kBlock), 0, s, d_in, n,
                       tmp.zero.data(), d_out);
    return;
  }
  if (level >= ScanTemp::kMaxLevels)
    throw std::runtime_error("scan: input too large");
  auto& bsums = tmp.sum_buf(level, nblocks);
  auto& boffs = tmp.off_buf(level, nblocks);
  hipLaunchKernelGGL(scan_pass_a<IN>, dim3(nblocks), dim3(kBlock), 0, s, d_in,
                     n, bsums.data());
  scan_recurse<uint64_t>(bsums.data(), boffs.data(), nblocks, s, tmp,
                         level + 1);
  hipLaunchKernelGGL(scan_pass_b<IN>, dim3(nblocks), dim3(kBlock), 0, s, d_in,
                     n, boffs.data(), d_out);
}

// Exclusive scan of n elements; d_out has n+1 slots (d_out[n] = total).
// Returns the total (host-synchronizing).
template <typename IN>
uint64_t exclusive_scan(const IN* d_in, uint64_t* d_out, size_t n,
                        hipStream_t s, ScanTemp& tmp) {
  if (n == 0) {
    uint64_t z = 0;
    HIP_CHECK(hipMemcpyAsync(d_out, &z, 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  }
  scan_recurse<IN>(d_in, d_out, n, s, tmp, 0);
  uint64_t last_off;
  IN last_in;
  HIP_CHECK(hipMemcpyAsync(&last_off, d_out + (n - 1), 8,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&last_in, d_in + (n - 1), sizeof(IN),
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  uint64_t total = last_off + static_cast<uint64_t>(last_in);
  HIP_CHECK(hipMemcpyAsync(d_out + n, &total, 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return total;
}

}  // namespace grapehip

namespace grapehip {

// ===========================================================================
// Small device helpers: queues, bitmaps, fills
// ===========================================================================

struct DevQueue {
  uint32_t* q;
  unsigned long long* cnt;
  __device__ __forceinline__ void push(uint32_t v) const {
    q[atomicAdd(cnt, 1ull)] = v;
  }
};

struct DevBitmap {
  uint32_t* words;
  __device__ __forceinline__ bool set_once(uint32_t v) const {
    uint32_t m = 1u << (v & 31);
    return (atomicOr(&words[v >> 5], m) & m) == 0;
  }
  __device__ __forceinline__ void clear_bit(uint32_t v) const {
    atomicAnd(&words[v >> 5], ~(1u << (v & 31)));
  }
};

template <typename T>
__global__ void fill_kernel(T* p, T v, size_t n) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < n; i += stride)
    p[i] = v;
}

template <typename T>
void fill(T* p, T v, size_t n, hipStream_t s) {
  if (n) fill_kernel<T><<<grid_for(n), kBlock, 0, s>>>(p, v, n);
}

__global__ void iota_kernel(uint32_t* p, uint32_t base, size_t n) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < n; i += stride)
    p[i] = base + static_cast<uint32_t>(i);
}

// ===========================================================================
// Synthetic generation (RMAT) + CSR build
// ===========================================================================

// Quadrant thresholds in 16-bit fixed point.
// scr_a/scr_b: bijective LCG scramble (gcd(scr_a,nv)=1) decorrelating
// RMAT's low-popcount hub ids from the contiguous ownership slices —
// without it rank 0 of an 8-way run owns ~45% of all edges (measured),
// which would sink the scaling curve. scr_a=0 disables.
__global__ void gen_edges_kernel(uint64_t ne, uint64_t seed, int scale,
                                 uint32_t nv, uint32_t t_a, uint32_t t_ab,
                                 uint32_t t_abc, uint64_t scr_a,
                                 uint64_t scr_b, uint32_t my_begin,
                                 uint32_t my_end, bool undirected,
                                 bool reverse, bool weighted,
                                 uint32_t* out_src, uint32_t* out_dst,
                                 float* out_w,
                                 unsigned long long* out_cnt) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < ne; i += stride) {
    uint64_t h = mix64(seed ^ (i * 0x9e3779b97f4a7c15ULL));
    uint32_t s = 0, d = 0;
    int avail = 0;
    uint64_t bits = 0;
    for (int b = 0; b < scale; ++b) {
      if (avail == 0) {
        bits = h;
        h = mix64(h + 0x632be59bd9b4e019ULL);
        avail = 4;
      }
      uint32_t r = static_cast<uint32_t>(bits & 0xFFFF);
      bits >>= 16;
      --avail;
      uint32_t quad = r < t_a ? 0u : (r < t_ab ? 1u : (r < t_abc ? 2u : 3u));
      s = (s << 1) | (quad >> 1);
      d = (d << 1) | (quad & 1);
    }
    if (s >= nv) s -= nv;  // fold 2^scale domain onto [0, nv)
    if (d >= nv) d -= nv;
    if (scr_a) {
      // LCG then swap {0, scr_b}: raw vertex 0 (the deepest RMAT hub)
      // keeps id 0, so the benchmark's named source stays the hub while
      // every slice still gets a uniform share of the edge mass
      uint64_t ss = (scr_a * s + scr_b) % nv;
      uint64_t dd = (scr_a * d + scr_b) % nv;
      s = static_cast<uint32_t>(ss == scr_b ? 0 : (ss == 0 ? scr_b : ss));
      d = static_cast<uint32_t>(dd == scr_b ? 0 : (dd == 0 ? scr_b : dd));
    }
    float w = 1.0f;
    if (weighted)
      w = static_cast<float>((h >> 16) & 0xFFFFFF) * (99.0f / 16777216.0f) +
          1.0f;
    // materialize both orientations for undirected storage; keep owned src.
    // reverse=true keeps edges by OWNED DST as (d, s) pairs — the same
    // deterministic edge stream builds the in-CSR of a directed graph.
    // out_src==nullptr: counting pass only (RMAT mass is skewed toward low
    // vids, so per-rank shares are NOT ne/world — rank 0 of an 8-way run
    // owns far more; exact counts size the buffers)
    if (!reverse && s >= my_begin && s < my_end) {
      uint64_t pos = atomicAdd(out_cnt, 1ull);
      if (out_src) {
        out_src[pos] = s;
        out_dst[pos] = d;
        if (weighted) out_w[pos] = w;
      }
    }
    if (undirected && d >= my_begin && d < my_end) {
      // self loops stored twice, like the reference's undirected CSR
      uint64_t pos = atomicAdd(out_cnt, 1ull);
      if (out_src) {
        out_src[pos] = d;
        out_dst[pos] = s;
        if (weighted) out_w[pos] = w;
      }
    }
    if (reverse && d >= my_begin && d < my_end) {
      uint64_t pos = atomicAdd(out_cnt, 1ull);
      if (out_src) {
        out_src[pos] = d;
        out_dst[pos] = s;
        if (weighted) out_w[pos] = w;
      }
    }
  }
}

// ===========================================================================
// Hub-clustering renumber. RMAT/power-law hot vertices are the ids with
// few set bits — scattered across the id range, so the pull kernels'
// contrib/label gathers fetch a cold 64B line per 4B value. Renumbering
// each slice by descending (capped) degree packs the hot ~1M vertices
// into a contiguous L2-resident prefix (measured: top-1M ids carry ~53%
// of endpoint references at datagen-9_0 shape, but only 8% sit in any
// contiguous 1M window). Owner-preserving: new id = v_begin + position
// within the slice, so slicing, halos and collectives are untouched.
// ===========================================================================

constexpr int kRenumBuckets = 4096;  // degree-capped counting sort

__global__ void renum_hist_kernel(const uint32_t* __restrict__ deg,
                                  uint32_t n,
                                  unsigned long long* __restrict__ hist) {
  __shared__ uint32_t h[kRenumBuckets];
  for (int b = threadIdx.x; b < kRenumBuckets; b += blockDim.x) h[b] = 0;
  __syncthreads();
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint32_t k = deg[i];
    atomicAdd(&h[k < kRenumBuckets ? k : kRenumBuckets - 1], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kRenumBuckets; b += blockDim.x)
    if (h[b]) atomicAdd(&hist[b], static_cast<unsigned long long>(h[b]));
}

// block-synchronous 3-phase scatter: LDS-aggregated cursor claims keep the
// hot low-degree buckets off the global atomic units
__global__ void renum_scatter_kernel(const uint32_t* __restrict__ deg,
                                     uint32_t n, uint32_t v_begin,
                                     unsigned long long* __restrict__ cur,
                                     uint32_t* __restrict__ perm) {
  __shared__ uint32_t h[kRenumBuckets];
  __shared__ unsigned long long base[kRenumBuckets];
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t chunk = blockIdx.x * blockDim.x; chunk < n;
       chunk += stride) {
    uint32_t i = chunk + threadIdx.x;
    uint32_t k = kRenumBuckets;
    if (i < n) {
      uint32_t d = deg[i];
      k = d < kRenumBuckets ? d : kRenumBuckets - 1;
    }
    for (int b = threadIdx.x; b < kRenumBuckets; b += blockDim.x) h[b] = 0;
    __syncthreads();
    uint32_t mypos = 0;
    if (k < kRenumBuckets) mypos = atomicAdd(&h[k], 1u);
    __syncthreads();
    for (int b = threadIdx.x; b < kRenumBuckets; b += blockDim.x)
      if (h[b])
        base[b] = atomicAdd(&cur[b], static_cast<unsigned long long>(h[b]));
    __syncthreads();
    if (k < kRenumBuckets)
      perm[v_begin + i] =
          v_begin + static_cast<uint32_t>(base[k] + mypos);
    __syncthreads();
  }
}

__global__ void remap_ids_kernel(uint32_t* __restrict__ ids, uint64_t n,
                                 const uint32_t* __restrict__ perm) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride)
    ids[i] = perm[ids[i]];
}

__global__ void inv_scatter_kernel(const uint32_t* __restrict__ perm,
                                   uint32_t n, uint32_t* __restrict__ inv) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    inv[perm[i]] = i;
}

__global__ void count_deg_kernel(const uint32_t* src, uint64_t n,
                                 uint32_t v_begin, uint32_t* deg) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride)
    atomicAdd(&deg[src[i] - v_begin], 1u);
}

__global__ void scatter_edges_kernel(const uint32_t* src, const uint32_t* dst,
                                     const float* w, uint64_t n,
                                     uint32_t v_begin,
                                     unsigned long long* cursor,
                                     uint32_t* out_dst, float* out_w) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride) {
    uint64_t pos = atomicAdd(&cursor[src[i] - v_begin], 1ull);
    out_dst[pos] = dst[i];
    if (w) out_w[pos] = w[i];
  }
}

// ===========================================================================
// Row tier partitioner, shared by the segmented sort, the pull-row buckets,
// the CDLP/LCC degree tiers and the LCC count tiers. A classifier maps row r
// to a bin: [0, kLists) appends r to that bin's list, [kLists, kBins) is only
// counted, a negative value drops the row. Order inside a list is
// unspecified.
//
// Block-aggregated: LDS tallies + one global reservation per block per bin
// (405M per-thread global atomics on 3 hot words took 4.8 s).
// ===========================================================================

template <int NLISTS>
struct TierListPtrs {
  uint32_t* p[NLISTS];
};

template <typename Classify>
__global__ void tier_rows_kernel(Classify cls, uint32_t rows_n,
                                 TierListPtrs<Classify::kLists> lists,
                                 unsigned long long* __restrict__ cnt) {
  constexpr int NBINS = Classify::kBins, NLISTS = Classify::kLists;
  __shared__ uint32_t s_cnt[NBINS];
  __shared__ unsigned long long s_base[NLISTS];
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t base = blockIdx.x * blockDim.x; base < rows_n;
       base += stride) {
    if (threadIdx.x < NBINS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t r = base + threadIdx.x;
    int b = -1;
    uint32_t loc = 0;
    if (r < rows_n) {
      b = cls(r);
      if (b >= 0) loc = atomicAdd(&s_cnt[b], 1u);
    }
    __syncthreads();
    if (threadIdx.x < NBINS && s_cnt[threadIdx.x]) {
      unsigned long long at =
          atomicAdd(cnt + threadIdx.x,
                    static_cast<unsigned long long>(s_cnt[threadIdx.x]));
      if (threadIdx.x < NLISTS) s_base[threadIdx.x] = at;
    }
    __syncthreads();
    if (b >= 0 && b < NLISTS) lists.p[b][s_base[b] + loc] = r;
    __syncthreads();
  }
}

// Partitions rows [0, rows_n) on stream s: sizes every non-null list for
// rows_n entries, launches, and reads the kBins counts back (one sync of s).
// A null list is for a bin the classifier never returns.
template <typename Classify>
std::vector<unsigned long long> partition_rows(
    Classify cls, uint32_t rows_n,
    DeviceBuffer<uint32_t>* const (&lists)[Classify::kLists],
    hipStream_t s) {
  TierListPtrs<Classify::kLists> ptrs;
  for (int b = 0; b < Classify::kLists; ++b) {
    if (lists[b]) lists[b]->resize(rows_n ? rows_n : 1);
    ptrs.p[b] = lists[b] ? lists[b]->data() : nullptr;
  }
  DeviceBuffer<unsigned long long> cnts(Classify::kBins);
  cnts.zero(s);
  if (rows_n)
    tier_rows_kernel<<<grid_for(rows_n), kBlock, 0, s>>>(cls, rows_n, ptrs,
                                                         cnts.data());
  return cnts.download(s);
}

// ===========================================================================
// Segmented sort (ascending keys per CSR row), shared by the adjacency sort
// of a freshly built device CSR and by LCC's oriented CSR. Ascending
// neighbor ids turn the pull kernels' random gathers into locally-increasing
// streams (L2-friendlier) and give deterministic adjacency order. A codec
// loads the key of row position i and stores it back; the padding key sorts
// last. LDS bitonic for rows <= kSegSortLds keys, pow2-padded global scratch
// bitonic for heavier rows.
// ===========================================================================

constexpr uint32_t kSegSortLds = 4096;  // 32 KB of LDS for u64, 16 KB for u32

// (dst, optional weight) pairs packed into u64, dst in the high half
struct PairKeyCodec {
  using Key = unsigned long long;
  static constexpr Key kPad = ~0ull;
  uint32_t* __restrict__ dst;
  float* __restrict__ w;  // null: unweighted
  __device__ __forceinline__ Key load(uint64_t i) const {
    return (static_cast<unsigned long long>(dst[i]) << 32) |
           (w ? __float_as_uint(w[i]) : 0u);
  }
  __device__ __forceinline__ void store(uint64_t i, Key k) const {
    dst[i] = static_cast<uint32_t>(k >> 32);
    if (w) w[i] = __uint_as_float(static_cast<uint32_t>(k));
  }
};

// plain u32 keys; vertex ids never reach the padding value
struct U32KeyCodec {
  using Key = uint32_t;
  static constexpr Key kPad = 0xFFFFFFFFu;
  uint32_t* __restrict__ dst;
  __device__ __forceinline__ Key load(uint64_t i) const { return dst[i]; }
  __device__ __forceinline__ void store(uint64_t i, Key k) const {
    dst[i] = k;
  }
};

template <typename Key>
__device__ __forceinline__ void bitonic_stage(Key* a, uint32_t n, uint32_t k,
                                              uint32_t j) {
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    uint32_t ij = i ^ j;
    if (ij > i) {
      bool up = (i & k) == 0;
      Key x = a[i], y = a[ij];
      if ((x > y) == up) {
        a[i] = y;
        a[ij] = x;
      }
    }
  }
}

// sort tiers by row length: LDS bitonic, global-scratch bitonic; rows of 0 or
// 1 keys need no sort and are in no tier
struct SortLenTiers {
  static constexpr int kLists = 2, kBins = 2;
  const uint64_t* __restrict__ off;
  __device__ __forceinline__ int operator()(uint32_t r) const {
    uint64_t n = off[r + 1] - off[r];
    return n < 2 ? -1 : (n <= kSegSortLds ? 0 : 1);
  }
};

template <typename Codec>
__global__ void seg_sort_lds_kernel(const uint64_t* __restrict__ off,
                                    Codec c,
                                    const uint32_t* __restrict__ rows,
                                    uint64_t nrows) {
  using Key = typename Codec::Key;
  __shared__ Key s_a[kSegSortLds];
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    uint64_t b = off[r];
    uint32_t n = static_cast<uint32_t>(off[r + 1] - b);
    uint32_t cap = 2;
    while (cap < n) cap <<= 1;
    for (uint32_t k = threadIdx.x; k < cap; k += blockDim.x)
      s_a[k] = k < n ? c.load(b + k) : Codec::kPad;
    __syncthreads();
    for (uint32_t k = 2; k <= cap; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        bitonic_stage(s_a, cap, k, j);
        __syncthreads();
      }
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x)
      c.store(b + k, s_a[k]);
    __syncthreads();
  }
}

__global__ void seg_bigcap_kernel(const uint64_t* __restrict__ off,
                                  const uint32_t* __restrict__ rows,
                                  uint64_t nrows,
                                  uint32_t* __restrict__ caps) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint64_t n = off[rows[i] + 1] - off[rows[i]];
    uint64_t cap = 2;
    while (cap < n) cap <<= 1;
    caps[i] = static_cast<uint32_t>(cap);
  }
}

template <typename Codec>
__global__ void seg_bigpad_kernel(const uint64_t* __restrict__ off, Codec c,
                                  const uint32_t* __restrict__ rows,
                                  uint64_t nrows,
                                  const uint64_t* __restrict__ pad_off,
                                  typename Codec::Key* __restrict__ scratch) {
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    uint64_t b = off[r];
    uint64_t n = off[r + 1] - b;
    uint64_t pb = pad_off[i];
    uint64_t cap = pad_off[i + 1] - pb;
    for (uint64_t k = threadIdx.x; k < cap; k += blockDim.x)
      scratch[pb + k] = k < n ? c.load(b + k) : Codec::kPad;
  }
}

template <typename Key>
__global__ void seg_bigsort_kernel(const uint64_t* __restrict__ pad_off,
                                   uint64_t nrows,
                                   Key* __restrict__ scratch) {
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint64_t pb = pad_off[i];
    uint32_t cap = static_cast<uint32_t>(pad_off[i + 1] - pb);
    Key* a = scratch + pb;
    for (uint32_t k = 2; k <= cap; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        bitonic_stage(a, cap, k, j);
        __syncthreads();
      }
  }
}

template <typename Codec>
__global__ void seg_bigunpad_kernel(const uint64_t* __restrict__ off, Codec c,
                                    const uint32_t* __restrict__ rows,
                                    uint64_t nrows,
                                    const uint64_t* __restrict__ pad_off,
                                    const typename Codec::Key* __restrict__
                                        scratch) {
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    uint64_t b = off[r];
    uint64_t n = off[r + 1] - b;
    uint64_t pb = pad_off[i];
    for (uint64_t k = threadIdx.x; k < n; k += blockDim.x)
      c.store(b + k, scratch[pb + k]);
  }
}

// ===========================================================================
// CM-style load-balanced edge expansion (LDS-staged owner search).
// Each block stages up to 256 consecutive work items (frontier entries or
// rows) with their frontier-edge prefix + adjacency base in LDS, then its
// 256 threads sweep the staged edges, binary-searching the owner in LDS.
// Reference semantics: cuda/parallel/parallel_engine.h LBCM (:718-771).
// ===========================================================================

// Default arcs per work item of expand_cm_frontier (GRAPEHIP_EXPAND_TILE
// overrides; see KERNELS.md "Tiled frontier expansion").
constexpr uint32_t kExpandTile = 4096;

// Last frontier entry i in [0, qn) with foff[i] <= e, for e < foff[qn]:
// the entry that owns arc e (entries without an arc repeat their
// successor's prefix and are never the last). One wave searches 64-ary,
// so 2^27 entries take five dependent loads, not 27. All 64 lanes call it.
__device__ __forceinline__ uint32_t wave_owner_search(
    const uint64_t* __restrict__ foff, uint32_t qn, uint64_t e, int lane) {
  uint64_t lo = 0, hi = qn;  // foff[lo] <= e; hi == qn or foff[hi] > e
  while (hi - lo > 1) {
    const uint64_t step = (hi - lo + 63) >> 6;
    const uint64_t p = lo + (lane + 1) * step;
    const bool le = p < hi && foff[p] <= e;
    // the prefix never decreases: the lanes that hold are lanes 0..cnt-1
    const int cnt = __popcll(__ballot(le));
    const uint64_t nlo = lo + cnt * step;
    const uint64_t nhi = nlo + step;
    lo = nlo;
    hi = nhi < hi ? nhi : hi;
  }
  return static_cast<uint32_t>(lo);
}

// Work item = tile of `tile` consecutive arcs of the frontier's arc space
// [0, total), not a count of entries: ascending-id queues put the heaviest
// rows first, and entry chunks gave a few blocks most of the arcs. A block
// finds the entry that owns its tile's first arc, then walks the owners in
// LDS batches of up to 256, sweeping each batch's arcs clamped to the tile.
// Every arc of [0, total) goes to op exactly once. Needs total > 0.
template <typename EdgeOp>
__global__ void expand_cm_frontier(DevGraphView g, const uint32_t* __restrict__ q,
                                   uint32_t qn, const uint64_t* __restrict__ foff,
                                   uint64_t total, uint32_t tile, EdgeOp op) {
  __shared__ uint64_t s_off[kBlock + 1];   // frontier-space edge prefix
  __shared__ uint64_t s_base[kBlock];      // CSR base of each vertex
  __shared__ uint32_t s_v[kBlock];
  __shared__ uint32_t s_first;
  const int tid = threadIdx.x;
  const uint64_t ntiles = (total + tile - 1) / tile;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t tile_lo = t * tile;
    const uint64_t tile_hi = tile_lo + tile < total ? tile_lo + tile : total;
    if (tid < kWave) {
      uint32_t first = wave_owner_search(foff, qn, tile_lo, tid);
      if (tid == 0) s_first = first;
    }
    __syncthreads();
    uint32_t chunk = s_first;
    for (;;) {
      const int n = min(static_cast<uint32_t>(kBlock), qn - chunk);
      if (tid < n) {
        const uint64_t o = foff[chunk + tid];
        s_off[tid] = o;
        // entries at or past the tile's end own none of its arcs
        if (o < tile_hi) {
          uint32_t v = q[chunk + tid];
          s_v[tid] = v;
          s_base[tid] = g.oe_off[g.row(v)];
        }
      }
      if (tid == 0) s_off[n] = foff[chunk + n];
      __syncthreads();
      const uint64_t batch_end = s_off[n];
      const uint64_t e0 = s_off[0] > tile_lo ? s_off[0] : tile_lo;
      const uint64_t e1 = batch_end < tile_hi ? batch_end : tile_hi;
      // a thread's edges are strided, so its owner index only moves forward:
      // binary-search once, then advance incrementally (amortized O(1) LDS)
      int lo = 0;
      {
        uint64_t e = e0 + tid;
        if (e < e1) {
          int hi = n - 1;
          while (lo < hi) {
            int mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= e) lo = mid; else hi = mid - 1;
          }
        }
      }
      for (uint64_t e = e0 + tid; e < e1; e += blockDim.x) {
        while (lo + 1 < n && s_off[lo + 1] <= e) ++lo;
        const uint32_t u = s_v[lo];
        const uint64_t eid = s_base[lo] + (e - s_off[lo]);
        op(u, g.oe_dst[eid], g.oe_w ? g.oe_w[eid] : 1.0f);
      }
      __syncthreads();
      if (batch_end >= tile_hi || chunk + n >= qn) break;
      chunk += n;
    }
  }
}

// Whole-owned-range variant (PR/WCC): work item i == row i; the global CSR
// offsets ARE the prefix — no frontier scan needed.
template <bool USE_IN, typename EdgeOp>
__global__ void expand_cm_range(DevGraphView g, EdgeOp op) {
  __shared__ uint64_t s_off[kBlock + 1];
  const int tid = threadIdx.x;
  const uint32_t rows = g.owned();
  const uint64_t* off = USE_IN ? g.ie_off : g.oe_off;
  const uint32_t* dst = USE_IN ? g.ie_dst : g.oe_dst;
  const float* wt = USE_IN ? g.ie_w : g.oe_w;
  for (uint32_t chunk = blockIdx.x * kBlock; chunk < rows;
       chunk += gridDim.x * kBlock) {
    const int n = min(static_cast<uint32_t>(kBlock), rows - chunk);
    if (tid < n) s_off[tid] = off[chunk + tid];
    if (tid == 0) s_off[n] = off[chunk + n];
    __syncthreads();
    const uint64_t e0 = s_off[0], e1 = s_off[n];
    int lo = 0;
    {
      uint64_t e = e0 + tid;
      if (e < e1) {
        int hi = n - 1;
        while (lo < hi) {
          int mid = (lo + hi + 1) >> 1;
          if (s_off[mid] <= e) lo = mid; else hi = mid - 1;
        }
      }
    }
    for (uint64_t e = e0 + tid; e < e1; e += blockDim.x) {
      while (lo + 1 < n && s_off[lo + 1] <= e) ++lo;
      op(g.v_begin + chunk + lo, dst[e], wt ? wt[e] : 1.0f);
    }
    __syncthreads();
  }
}

// STRICT load balancing (reference cuda/parallel/parallel_engine.h
// LBSTRICT :883-979): perfectly edge-balanced — every block owns exactly
// ceil(total/grid) edge outputs regardless of row skew. Row ownership is
// found by binary search in the frontier edge prefix; the search is
// re-anchored once per thread and advanced incrementally (a thread's
// edges are strided, so its owner only moves forward).
__device__ __forceinline__ uint32_t strict_owner(
    const uint64_t* __restrict__ foff, uint32_t qn, uint64_t e) {
  uint32_t lo = 0, hi = qn;  // find last row with foff[row] <= e
  while (lo + 1 < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (foff[mid] <= e)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

template <typename EdgeOp>
__global__ void expand_strict_frontier(DevGraphView g,
                                       const uint32_t* __restrict__ q,
                                       uint32_t qn,
                                       const uint64_t* __restrict__ foff,
                                       uint64_t total, EdgeOp op) {
  uint64_t per = (total + gridDim.x - 1) / gridDim.x;
  uint64_t eb = per * blockIdx.x;
  if (eb >= total) return;
  uint64_t ee = eb + per < total ? eb + per : total;
  uint64_t e = eb + threadIdx.x;
  if (e >= ee) return;
  uint32_t owner = strict_owner(foff, qn, e);
  for (; e < ee; e += blockDim.x) {
    while (owner + 1 < qn && foff[owner + 1] <= e) ++owner;
    uint32_t u = q[owner];
    uint64_t eid = g.oe_off[g.row(u)] + (e - foff[owner]);
    op(u, g.oe_dst[eid], g.oe_w ? g.oe_w[eid] : 1.0f);
  }
}

// WM: wave-granular CM (reference LBWARP, parallel_engine.h:775-845,
// re-derived for 64-wide waves). Each wave claims 64 frontier entries and
// stages their adjacency bases + degree prefix in REGISTERS (no LDS):
// the prefix comes from a wave inclusive scan, owner search probes
// lane-held prefix values with __shfl (6-step binary search per edge).
template <typename EdgeOp>
__global__ void expand_wm_frontier(DevGraphView g,
                                   const uint32_t* __restrict__ q,
                                   uint32_t qn, EdgeOp op) {
  const int lane = threadIdx.x & 63;
  const uint64_t wid =
      (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) /
      kWave;
  const uint64_t waves =
      (static_cast<uint64_t>(gridDim.x) * blockDim.x) / kWave;
  for (uint64_t c = wid * kWave; c < qn; c += waves * kWave) {
    uint32_t i = static_cast<uint32_t>(c) + lane;
    bool act = i < qn;
    uint32_t u = act ? q[i] : 0;
    uint64_t b = 0;
    uint32_t deg = 0;
    if (act) {
      uint32_t r = g.row(u);
      b = g.oe_off[r];
      deg = static_cast<uint32_t>(g.oe_off[r + 1] - b);
    }
    uint64_t incl = wave_incl_scan(deg);
    uint64_t total = __shfl(static_cast<unsigned long long>(incl), 63, 64);
    uint64_t excl = incl - deg;
    // whole-wave trips: the probes below read other lanes' registers, and
    // a lane that had left the loop (last trip of a chunk whose edge count
    // is no multiple of 64) holds no defined answer
    for (uint64_t e0 = 0; e0 < total; e0 += kWave) {
      const uint64_t e = e0 + lane;
      int lo = 0, hi = 63;
#pragma unroll
      for (int step = 0; step < 6; ++step) {
        int mid = (lo + hi + 1) >> 1;
        uint64_t px =
            __shfl(static_cast<unsigned long long>(excl), mid, 64);
        if (px <= e) lo = mid;
        else hi = mid - 1;
      }
      uint32_t uo = __shfl(u, lo, 64);
      uint64_t bo = __shfl(static_cast<unsigned long long>(b), lo, 64);
      uint64_t po = __shfl(static_cast<unsigned long long>(excl), lo, 64);
      if (e < total) {
        uint64_t eid = bo + (e - po);
        op(uo, g.oe_dst[eid], g.oe_w ? g.oe_w[eid] : 1.0f);
      }
    }
  }
}

// Thread-per-item baseline (LB=none), frontier form.
template <typename EdgeOp>
__global__ void expand_none_frontier(DevGraphView g,
                                     const uint32_t* __restrict__ q,
                                     uint32_t qn, EdgeOp op) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < qn;
       i += stride) {
    uint32_t u = q[i];
    uint32_t r = g.row(u);
    uint64_t b = g.oe_off[r], e = g.oe_off[r + 1];
    for (uint64_t k = b; k < e; ++k)
      op(u, g.oe_dst[k], g.oe_w ? g.oe_w[k] : 1.0f);
  }
}

__global__ void gather_deg_kernel(DevGraphView g, const uint32_t* q,
                                  uint32_t qn, uint32_t* deg) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < qn;
       i += stride) {
    uint32_t r = g.row(q[i]);
    deg[i] = static_cast<uint32_t>(g.oe_off[r + 1] - g.oe_off[r]);
  }
}

}  // namespace grapehip

namespace grapehip {

// ===========================================================================
// Halo exchange (the GPUMessageManager, MI355X-shaped).
// Appends are deduped through a global-vid bitmap; per-peer index regions are
// packed into (v, state[v]) pairs at flush and exchanged with paired
// ncclSend/ncclRecv over xGMI; lengths travel on the TCP control plane.
// ===========================================================================

template <typename T>
struct HaloPair {
  uint32_t v;
  T val;
};

struct DevHalo {
  uint32_t* idx;                 // [world * cap]
  unsigned long long* cnt;       // [world]
  DevBitmap bm;                  // global-vid dedup
  uint64_t cap;
  uint32_t slice;
  int world;
  __device__ __forceinline__ void add(uint32_t v) const {
    if (bm.set_once(v)) {
      uint32_t o = v / slice;
      if (static_cast<int>(o) >= world) o = world - 1;
      idx[o * cap + atomicAdd(&cnt[o], 1ull)] = v;
    }
  }
};

template <typename T>
__global__ void halo_pack_kernel(const uint32_t* __restrict__ idx, uint64_t n,
                                 const T* __restrict__ state, DevBitmap bm,
                                 HaloPair<T>* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride) {
    uint32_t v = idx[i];
    out[i].v = v;
    out[i].val = state[v];
    bm.clear_bit(v);
  }
}

// Take-and-zero pack for accumulated state (k-core decrement counts): ships
// (v, state[v]) and leaves state[v] == 0 for the next flush. No adder runs
// concurrently (the expansion kernel precedes it on the stream), so a plain
// read + store suffices.
template <typename T>
__global__ void halo_pack_take_kernel(const uint32_t* __restrict__ idx,
                                      uint64_t n, T* __restrict__ state,
                                      DevBitmap bm,
                                      HaloPair<T>* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride) {
    uint32_t v = idx[i];
    out[i].v = v;
    out[i].val = state[v];
    state[v] = T(0);
    bm.clear_bit(v);
  }
}

template <typename T, typename Op>
__global__ void halo_process_kernel(const HaloPair<T>* __restrict__ pairs,
                                    uint64_t n, Op op) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride)
    op(pairs[i].v, pairs[i].val);
}

__global__ void clear_bits_kernel(const uint32_t* __restrict__ q, uint32_t n,
                                  DevBitmap bm) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    bm.clear_bit(q[i]);
}

// ===========================================================================
// Bitmap frontier compaction: mark bits during expansion (1 atomicOr per
// improvement instead of bitmap+queue atomics), then popc+scan+fill to
// materialize the queue. Clears the bitmap as it fills.
// ===========================================================================

__global__ void popc_words_kernel(const uint32_t* __restrict__ words,
                                  size_t nwords, uint32_t* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < nwords; i += stride)
    out[i] = __popc(words[i]);
}

__global__ void fill_frontier_kernel(uint32_t* __restrict__ words,
                                     size_t nwords,
                                     const uint64_t* __restrict__ woff,
                                     uint32_t bit_base,
                                     uint32_t* __restrict__ q) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < nwords; i += stride) {
    uint32_t bits = words[i];
    if (!bits) continue;
    uint64_t base = woff[i];
    while (bits) {
      int b = __builtin_ctz(bits);
      bits &= bits - 1;
      q[base++] = bit_base + (static_cast<uint32_t>(i) << 5) + b;
    }
    words[i] = 0;
  }
}

// ===========================================================================
// App edge-op functors
// ===========================================================================

struct BfsOp {
  uint32_t* depth;
  uint32_t next_depth;
  DevBitmap next_bm;  // over owned bits
  uint32_t v_begin, v_end;
  bool multi;
  DevHalo halo;
  __device__ __forceinline__ void operator()(uint32_t, uint32_t d,
                                             float) const {
    // cheap cached read first: most edges hit settled vertices
    if (depth[d] <= next_depth) return;
    if (atomicMin(&depth[d], next_depth) > next_depth) {
      if (d >= v_begin && d < v_end)
        next_bm.set_once(d - v_begin);
      else if (multi)
        halo.add(d);
    }
  }
};

struct BfsRecvOp {  // incoming (v, depth) — v owned here
  uint32_t* depth;
  DevBitmap next_bm;
  uint32_t v_begin;
  __device__ __forceinline__ void operator()(uint32_t v, uint32_t dv) const {
    if (atomicMin(&depth[v], dv) > dv) next_bm.set_once(v - v_begin);
  }
};

__global__ void bfs_seed_kernel(uint32_t* depth, uint32_t src,
                                uint32_t v_begin, uint32_t* bm_words) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    depth[src] = 0;
    uint32_t r = src - v_begin;
    bm_words[r >> 5] |= 1u << (r & 31);
  }
}

// ---------------------------------------------------------------------------
// Betweenness centrality (single-source Brandes; cpp/apps/bc.hpp semantics).
// depth/sigma/acc are indexed by global vid. Owned entries hold the vertex's
// state; on several ranks the remote entries of sigma and acc hold this
// rank's pending contributions, zero between halo flushes. The fp64 adds
// are the hardware atomic (hipMalloc memory only).
// ---------------------------------------------------------------------------

// Forward arc v->u at level next_depth - 1. Every arc from the previous
// level into a vertex first reached at next_depth adds the tail's path
// count; the one that lowered the depth also queues the vertex. sigma[v]
// was completed by the previous level's launch.
struct BcFwdOp {
  uint32_t* depth;
  double* sigma;
  uint32_t next_depth;
  DevBitmap next_bm;  // over owned bits
  uint32_t v_begin, v_end;
  bool multi;
  DevHalo halo;
  __device__ __forceinline__ void operator()(uint32_t v, uint32_t u,
                                             float) const {
    // cheap cached read first: settled vertices (self-loops among them)
    if (depth[u] < next_depth) return;
    const bool own = u >= v_begin && u < v_end;
    if (!own && !multi) return;
    uint32_t old = atomicMin(&depth[u], next_depth);
    if (old < next_depth) return;
    unsafeAtomicAdd(&sigma[u], sigma[v]);
    if (own) {
      if (old > next_depth) next_bm.set_once(u - v_begin);
    } else {
      halo.add(u);
    }
  }
};

// incoming (v, path count) of the level being expanded — v owned here. The
// owner applies the sender's rule: a sender's depth copy is an upper bound,
// so a pair for a vertex that is already shallower is dropped.
struct BcFwdRecvOp {
  uint32_t* depth;
  double* sigma;
  uint32_t next_depth;
  DevBitmap next_bm;
  uint32_t v_begin;
  __device__ __forceinline__ void operator()(uint32_t v, double sig) const {
    if (depth[v] < next_depth) return;
    uint32_t old = atomicMin(&depth[v], next_depth);
    if (old < next_depth) return;
    unsafeAtomicAdd(&sigma[v], sig);
    if (old > next_depth) next_bm.set_once(v - v_begin);
  }
};

// Backward arc v->u, v at depth up_depth + 1: push v's coefficient to the
// shallower end (the reference's out-adjacency rule, directed or not).
struct BcBackOp {
  const uint32_t* depth;
  const double* coef;  // by owned row
  double* acc;
  uint32_t up_depth;
  uint32_t v_begin, v_end;
  bool multi;
  DevHalo halo;
  __device__ __forceinline__ void operator()(uint32_t v, uint32_t u,
                                             float) const {
    if (depth[u] != up_depth) return;
    const bool own = u >= v_begin && u < v_end;
    if (!own && !multi) return;
    unsafeAtomicAdd(&acc[u], coef[v - v_begin]);
    if (!own) halo.add(u);
  }
};

struct BcBackRecvOp {  // incoming (v, coefficient sum) — v owned here
  double* acc;
  __device__ __forceinline__ void operator()(uint32_t v, double c) const {
    unsafeAtomicAdd(&acc[v], c);  // several peers may send the same v
  }
};

__global__ void bc_seed_kernel(uint32_t* depth, double* sigma, uint32_t src,
                               uint32_t v_begin, uint32_t* bm_words) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    depth[src] = 0;
    sigma[src] = 1.0;
    uint32_t r = src - v_begin;
    bm_words[r >> 5] |= 1u << (r & 31);
  }
}

// One level's slice of the order array, after every deeper level has been
// expanded: delta = sigma * acc (kept in acc) and the coefficient the
// level's arcs push upwards. sigma >= 1 for every queued vertex.
__global__ void bc_finalize_kernel(const uint32_t* __restrict__ q,
                                   uint32_t qn, uint32_t v_begin,
                                   const double* __restrict__ sigma,
                                   double* __restrict__ acc,
                                   double* __restrict__ coef) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < qn;
       i += stride) {
    uint32_t v = q[i];
    double s = sigma[v];
    double dl = s * acc[v];
    acc[v] = dl;
    coef[v - v_begin] = (1.0 + dl) / s;
  }
}

struct SsspOp {
  float* dist;
  float prio_hi;
  DevBitmap near_bm;  // over owned bits; compacted to a queue per round
  DevQueue far_q;
  DevBitmap far_bm;  // over global vids (dedup across rounds)
  uint32_t v_begin, v_end;
  bool multi;
  DevHalo halo;
  __device__ __forceinline__ void bucket(uint32_t d, float nd) const {
    if (d >= v_begin && d < v_end) {
      if (nd < prio_hi) {
        near_bm.set_once(d - v_begin);
      } else {
        if (far_bm.set_once(d)) far_q.push(d);
      }
    } else if (multi) {
      halo.add(d);
    }
  }
  __device__ __forceinline__ void operator()(uint32_t u, uint32_t d,
                                             float w) const {
    float nd = dist[u] + w;
    if (dist[d] <= nd) return;  // cached read gate before the atomic
    float old = atomicMinPosFloat(&dist[d], nd);
    if (nd < old) bucket(d, nd);
  }
};

struct SsspRecvOp {
  float* dist;
  float prio_hi;
  DevBitmap near_bm;
  DevQueue far_q;
  DevBitmap far_bm;
  uint32_t v_begin;
  __device__ __forceinline__ void operator()(uint32_t v, float dv) const {
    float old = atomicMinPosFloat(&dist[v], dv);
    if (dv < old) {
      if (dv < prio_hi) {
        near_bm.set_once(v - v_begin);
      } else {
        if (far_bm.set_once(v)) far_q.push(v);
      }
    }
  }
};

__global__ void sssp_seed_kernel(float* dist, uint32_t src, uint32_t v_begin,
                                 uint32_t* near_words) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    dist[src] = 0.0f;
    uint32_t r = src - v_begin;
    near_words[r >> 5] |= 1u << (r & 31);
  }
}

// far-queue repartition after a priority advance
__global__ void sssp_repart_kernel(const uint32_t* __restrict__ far_in,
                                   uint32_t n, const float* __restrict__ dist,
                                   float prio_hi, DevBitmap near_bm,
                                   uint32_t v_begin, DevQueue far_out,
                                   DevBitmap far_bm) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint32_t v = far_in[i];
    if (dist[v] < prio_hi) {
      far_bm.clear_bit(v);
      near_bm.set_once(v - v_begin);
    } else {
      far_out.push(v);  // keeps its far bit
    }
  }
}

struct PrPushOp {
  const float* __restrict__ contrib;  // per owned row
  double* acc;
  uint32_t v_begin;
  __device__ __forceinline__ void operator()(uint32_t u, uint32_t d,
                                             float) const {
    unsafeAtomicAdd(&acc[d], static_cast<double>(contrib[u - v_begin]));
  }
};

// fp32 contributions (the reference's GPU PageRank precision,
// cuda/pagerank/pagerank.h:27-35 rank_t=float): halves the random-gather
// bytes of the pull pass; the rank/accumulator side stays fp64.
__global__ void pr_contrib_kernel(const double* __restrict__ rank,
                                  const uint64_t* __restrict__ off,
                                  uint32_t owned, uint32_t v_begin,
                                  float* __restrict__ contrib) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride) {
    uint64_t deg = off[r + 1] - off[r];
    contrib[r] = deg ? static_cast<float>(rank[v_begin + r] /
                                          static_cast<double>(deg))
                     : 0.0f;
  }
}

// The per-iteration scalar, a row's new rank and its next contribution. One
// text each for pr_fused_apply_kernel and the pull epilogues, so that the
// contraction into fused multiply-adds cannot differ between the two paths.
__device__ __forceinline__ double pr_base_of(double damping, double inv_n,
                                             double dangling) {
  return (1.0 - damping) * inv_n + damping * dangling * inv_n;
}

__device__ __forceinline__ double pr_new_rank(double base, double damping,
                                              double sum) {
  return base + damping * sum;
}

__device__ __forceinline__ float pr_contrib_of(double nv, uint64_t deg) {
  return static_cast<float>(nv / static_cast<double>(deg));
}

__global__ void pr_apply_kernel(double* __restrict__ rank,
                                const double* __restrict__ acc,
                                const double* __restrict__ dangling,
                                double inv_n, double damping,
                                uint32_t v_begin, uint32_t owned,
                                double* __restrict__ l1_delta) {
  __shared__ double s_wave[kBlock / kWave];
  // base recomputed on device so the whole iteration is hipGraph-capturable
  const double base =
      (1.0 - damping) * inv_n + damping * (*dangling) * inv_n;
  double d1 = 0;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride) {
    double nv = base + damping * acc[v_begin + r];
    if (l1_delta) d1 += fabs(nv - rank[v_begin + r]);
    rank[v_begin + r] = nv;
  }
  if (!l1_delta) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) d1 += __shfl_down(d1, d, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = d1;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) t += s_wave[w];
    unsafeAtomicAdd(l1_delta, t);
  }
}

// Fused apply + NEXT iteration's contrib/dangling: one pass over rank
// and the out-degree offsets instead of three (apply, then contrib, then
// dangling each re-reading rank). Single-GPU pull path; rows beyond
// owned_real (hashmap padding) get the rank update only.
//
// Only the active rows (rows_active: an edge in the pull or the out-CSR)
// are visited. An isolated row's acc is 0, so its rank is exactly `base`
// every iteration: the whole isolated population is carried by scalars.
// Thread 0 of block 0 adds n_isolated * base to the next dangling sum and
// n_isolated * |base - previous base| to the L1 delta, then stores base in
// *prev_base (read and written by that thread alone; the first iteration
// finds 1/N there). pr_fill_isolated_kernel writes the last base into
// the isolated rows' ranks after the loop.
__global__ void pr_fused_apply_kernel(
    double* __restrict__ rank, const double* __restrict__ acc,
    const double* __restrict__ dangling_cur, double inv_n, double damping,
    uint32_t v_begin, const uint32_t* __restrict__ rows, uint64_t nrows,
    uint32_t owned_real, double n_isolated, double* __restrict__ prev_base,
    const uint64_t* __restrict__ off, float* __restrict__ contrib,
    double* __restrict__ dangling_next, double* __restrict__ l1_delta) {
  __shared__ double s_wave[kBlock / kWave];
  __shared__ double s_dang[kBlock / kWave];
  const double base = pr_base_of(damping, inv_n, *dangling_cur);
  double d1 = 0, dang = 0;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint32_t r = rows[i];
    double nv = pr_new_rank(base, damping, acc[v_begin + r]);
    if (l1_delta) d1 += fabs(nv - rank[v_begin + r]);
    rank[v_begin + r] = nv;
    if (r < owned_real) {
      uint64_t deg = off[r + 1] - off[r];
      if (deg) {
        contrib[r] = pr_contrib_of(nv, deg);
      } else {
        contrib[r] = 0.0f;
        dang += nv;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dang += n_isolated * base;
    if (l1_delta) d1 += n_isolated * fabs(base - *prev_base);
    *prev_base = base;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    dang += __shfl_down(dang, d, 64);
    if (l1_delta) d1 += __shfl_down(d1, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_dang[threadIdx.x >> 6] = dang;
    s_wave[threadIdx.x >> 6] = d1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double td = 0, t1 = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
      td += s_dang[w];
      t1 += s_wave[w];
    }
    if (td) unsafeAtomicAdd(dangling_next, td);
    if (l1_delta && t1) unsafeAtomicAdd(l1_delta, t1);
  }
}

__global__ void pr_dangling_kernel(const double* __restrict__ rank,
                                   const uint64_t* __restrict__ off,
                                   uint32_t owned, uint32_t v_begin,
                                   double* __restrict__ out) {
  __shared__ double s_wave[kBlock / kWave];
  double sum = 0;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride)
    if (off[r + 1] == off[r]) sum += rank[v_begin + r];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) t += s_wave[w];
    unsafeAtomicAdd(out, t);
  }
}

// ---------------------------------------------------------------------------
// PageRank epilogues (undirected graph, single GPU, fixed iterations; see
// GpuContext::pagerank_epilogue and KERNELS.md). A pull that has a row's sum
// in hand applies it on the spot instead of storing it to acc for
// pr_fused_apply_kernel to read back: EPI 0 stores the sum (every other
// path), EPI 1 writes the row's next contribution, EPI 2, on the last
// iteration, its rank. Every active row of an undirected graph has a pull
// edge, so none is dangling and the dangling sum is the isolated rows'
// alone: a scalar recurrence, stepped by one thread.
// ---------------------------------------------------------------------------
struct PrEpilogue {
  const double* base;   // pr_epi_scal + 1, written by pr_epi_scalar_kernel
  double damping;
  float* contrib_next;  // by stored id, EPI 1
  double* rank;         // by stored id, EPI 2
};

template <int EPI>
__device__ __forceinline__ void pr_row_done(const PrEpilogue& ep, double base,
                                            uint32_t v, double sum,
                                            uint64_t deg) {
  const double nv = pr_new_rank(base, ep.damping, sum);
  if (EPI == 1) ep.contrib_next[v] = pr_contrib_of(nv, deg);
  else ep.rank[v] = nv;
}

// sc: [0]=dangling sum, [1]=base, [2]=previous base. What thread 0 of
// pr_fused_apply_kernel does with the isolated rows, and nothing else.
__global__ void pr_epi_scalar_kernel(double* __restrict__ sc, double inv_n,
                                     double damping, double n_isolated) {
  const double base = pr_base_of(damping, inv_n, sc[0]);
  sc[1] = base;
  sc[0] = n_isolated * base;
  sc[2] = base;
}

// Start of a call: every rank is 1/N, so the dangling sum is a count times
// 1/N and a row's contribution is (1/N)/deg.
__global__ void pr_epi_init_kernel(double* __restrict__ sc, double dangling0,
                                   double inv_n) {
  sc[0] = dangling0;
  sc[1] = inv_n;
  sc[2] = inv_n;
}

__global__ void pr_epi_contrib0_kernel(const uint32_t* __restrict__ rows,
                                       uint64_t nrows,
                                       const uint64_t* __restrict__ off,
                                       double inv_n, uint32_t v_begin,
                                       float* __restrict__ contrib) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    const uint32_t r = rows[i];
    const uint64_t deg = off[r + 1] - off[r];
    contrib[v_begin + r] = deg ? pr_contrib_of(inv_n, deg) : 0.0f;
  }
}

// WCC: min-root union-find with path halving (Afforest-style hooks).
__device__ __forceinline__ uint32_t wcc_find(uint32_t* parent, uint32_t v) {
  for (;;) {
    uint32_t p = parent[v];
    if (p == v) return v;
    uint32_t gp = parent[p];
    if (gp == p) return p;
    // path halving MUST be monotone: a plain store can overwrite a
    // concurrently-lowered entry with a stale-derived higher value — or
    // even re-self-root it (gp read stale == v), severing a hook link
    // and splitting the component (seen at 1M-vertex scale)
    atomicMin(&parent[v], gp);
    v = gp;
  }
}

struct WccOp {
  uint32_t* parent;
  int* changed;
  uint32_t* mark_words;  // multi-GPU: entries hooked this round (for the
                         // sparse pair merge); nullptr on one GPU
  __device__ __forceinline__ void operator()(uint32_t u, uint32_t v,
                                             float) const {
    for (;;) {
      uint32_t ru = wcc_find(parent, u);
      uint32_t rv = wcc_find(parent, v);
      if (ru == rv) return;
      uint32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
      uint32_t old = atomicCAS(&parent[hi], hi, lo);
      if (old == hi) {
        *changed = 1;
        if (mark_words)
          atomicOr(&mark_words[hi >> 5], 1u << (hi & 31));
        return;
      }
      // CAS returned the CURRENT entry — chase from it rather than
      // re-reading parent[hi] (a stale cached line would spin forever)
      u = old;
      v = lo;
    }
  }
};

__global__ void wcc_compress_kernel(uint32_t* parent, uint32_t n,
                                    int* changed = nullptr) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n;
       v += stride) {
    uint32_t r = wcc_find(parent, v);
    if (parent[v] != r) {
      atomicMin(&parent[v], r);  // monotone (see wcc_find)
      if (changed) *changed = 1;
    }
  }
}

// Output canonicalization. wcc_find's path-halving store races
// non-monotonically (a stale-derived higher value can overwrite a
// concurrently lowered entry), so a "no-change" wcc_compress pass can
// still leave entries pointing at non-roots. This variant chases
// READ-ONLY and writes only true static-forest roots — two clean passes
// guarantee parent[v] == root(v) exactly.
__global__ void wcc_finalize_kernel(uint32_t* __restrict__ parent,
                                    uint32_t n, int* __restrict__ changed) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n;
       v += stride) {
    uint32_t r = v;
    uint32_t p;
    while ((p = parent[r]) != r) r = p;
    if (parent[v] != r) {
      parent[v] = r;
      *changed = 1;
    }
  }
}

// pack (v, parent[v]) pairs for the sparse multi-GPU merge
__global__ void wcc_pack_pairs_kernel(const uint32_t* __restrict__ q,
                                      uint64_t n,
                                      const uint32_t* __restrict__ parent,
                                      uint32_t* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride) {
    uint32_t v = q[i];
    out[2 * i] = v;
    out[2 * i + 1] = parent[v];
  }
}

__global__ void wcc_apply_pairs_kernel(const uint32_t* __restrict__ pairs,
                                       uint64_t n, uint64_t skip_b,
                                       uint64_t skip_e,
                                       uint32_t* __restrict__ parent) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride) {
    if (i >= skip_b && i < skip_e) continue;  // own pairs already applied
    atomicMin(&parent[pairs[2 * i]], pairs[2 * i + 1]);
  }
}

// Afforest-style neighbor sampling (Sutton et al.): hook only the first K
// edges of each row — a cheap streaming pass that already collapses most
// of a power-law graph into its giant component.
__global__ void wcc_sample_kernel(DevGraphView g, int which,
                                  uint32_t* parent, int* changed,
                                  uint32_t* mark_words) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const uint32_t rows = g.owned();
  WccOp op{parent, changed, mark_words};
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows;
       r += stride) {
    uint64_t b = g.oe_off[r], e = g.oe_off[r + 1];
    uint64_t i = b + which;
    if (i < e) op(g.v_begin + r, g.oe_dst[i], 1.0f);
  }
}

// mark owned rows NOT in the giant component (bitmap -> frontier queue);
// their remaining edges are the only ones the full pass must visit
__global__ void wcc_mark_rest_kernel(const uint32_t* __restrict__ parent,
                                     const uint64_t* __restrict__ off,
                                     uint32_t owned, uint32_t v_begin,
                                     uint32_t giant, DevBitmap bm) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride)
    if (parent[v_begin + r] != giant && off[r + 1] != off[r])
      bm.set_once(r);
}

// ===========================================================================
// k-core / core decomposition by level-synchronous frontier peeling.
// Reference parity: examples/analytical_apps/kcore/kcore.h and
// core_decomposition/core_decomposition.h (the reference runs both on the
// CPU only). Semantics are cpp/apps/kcore.hpp's: residual degree = stored
// out-CSR row length with multiplicity, self-loops excluded; peeling a
// vertex decrements each stored out-neighbour once per arc.
// deg/core are indexed by owned row; deg is signed so a peeled vertex may
// keep falling below its level. core[r] < 0 means "not peeled yet".
// ===========================================================================

// deg[r] = row length. Rows of 2^31 arcs or more raise *too_long (the host
// throws); the owner-searched self-loop sweep below does the correction, so
// no thread walks a row here.
__global__ void kcore_init_deg_kernel(const uint64_t* __restrict__ off,
                                      uint32_t owned, int* __restrict__ deg,
                                      int* __restrict__ too_long) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride) {
    uint64_t len = off[r + 1] - off[r];
    if (len > static_cast<uint64_t>(INT_MAX)) *too_long = 1;
    deg[r] = static_cast<int>(len);
  }
}

// expand_cm_range op: one decrement per stored self-loop arc
struct KcoreSelfLoopOp {
  int* deg;
  uint32_t v_begin;
  __device__ __forceinline__ void operator()(uint32_t u, uint32_t d,
                                             float) const {
    if (d == u) atomicSub(&deg[u - v_begin], 1);
  }
};

// min residual degree over the rows not yet peeled (INT_MAX if none):
// wave64 shuffle, LDS across the block's waves, one atomicMin per block
__global__ void kcore_min_alive_kernel(const int* __restrict__ deg,
                                       const int* __restrict__ core,
                                       uint32_t rows, int* __restrict__ out) {
  __shared__ int s_wave[kBlock / kWave];
  int m = INT_MAX;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows;
       r += stride)
    if (core[r] < 0) m = min(m, deg[r]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = min(m, __shfl_down(m, d, 64));
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = INT_MAX;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) t = min(t, s_wave[w]);
    if (t != INT_MAX) atomicMin(out, t);
  }
}

// Seed the (all-zero) owned-row bitmap with the unpeeled rows at or below
// the level. One lane per row; a wave ballots its 64 rows into two whole
// bitmap words, so no atomics. Every lane of a wave runs the same trips
// (the stride is a multiple of 64 and the bound is on the wave's base row).
__global__ void kcore_seed_kernel(const int* __restrict__ deg,
                                  const int* __restrict__ core,
                                  uint32_t rows, int level,
                                  uint32_t* __restrict__ bm_words) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                       (threadIdx.x - lane);
       base < rows; base += stride) {
    uint64_t r = base + lane;
    bool hit = r < rows && core[r] < 0 && deg[r] <= level;
    unsigned long long mask = __ballot(hit);
    if (lane == 0)
      bm_words[base >> 5] = static_cast<uint32_t>(mask);
    else if (lane == 32 && r < rows)
      bm_words[r >> 5] = static_cast<uint32_t>(mask >> 32);
  }
}

// record the level of every queued vertex (seeds and crossers alike)
__global__ void kcore_stamp_kernel(const uint32_t* __restrict__ q,
                                   uint32_t qn, uint32_t v_begin, int level,
                                   int* __restrict__ core) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < qn;
       i += stride)
    core[q[i] - v_begin] = level;
}

// Peel arc u->d. The crossing test (old above the level, new at or below
// it) fires for exactly one decrement per vertex, so each vertex enters a
// frontier once with no separate alive check: vertices already peeled or
// already queued sit at or below the level and can never cross again.
struct KcoreOp {
  int* deg;
  int level;
  DevBitmap next_bm;  // over owned bits
  uint32_t v_begin, v_end;
  bool multi;
  uint32_t* dec;  // multi-rank: pending decrements per remote vertex
  DevHalo halo;
  __device__ __forceinline__ void operator()(uint32_t u, uint32_t d,
                                             float) const {
    if (d == u) return;
    if (d >= v_begin && d < v_end) {
      int old = atomicSub(&deg[d - v_begin], 1);
      if (old > level && old - 1 <= level) next_bm.set_once(d - v_begin);
    } else if (multi) {
      atomicAdd(&dec[d], 1u);
      halo.add(d);
    }
  }
};

struct KcoreRecvOp {  // incoming (v, count) — v owned here
  int* deg;
  int level;
  DevBitmap next_bm;
  uint32_t v_begin;
  __device__ __forceinline__ void operator()(uint32_t v, uint32_t c) const {
    // c counts arcs into v, fewer than 2^31 (the driver checks)
    int ci = static_cast<int>(c);
    int old = atomicSub(&deg[v - v_begin], ci);
    if (old > level && old - ci <= level) next_bm.set_once(v - v_begin);
  }
};

}  // namespace grapehip

namespace grapehip {

// ===========================================================================
// Degree-bucketed row scheduler + pull-PageRank kernels.
// Pull (gather) PageRank has NO atomics: with undirected symmetric storage
// (or the in-CSR for directed graphs) every owned row's full neighborhood is
// local, so each row's accumulator is a private sum — the fp64-atomic push
// was 10x slower at datagen-9_0 scale. Rows are bucketed by degree once:
// thread-per-row (1..63), wave-per-row (<16384), block per 4096-arc segment
// (rest); rows without a pull edge are in no bucket — the
// preprocessed analogue of the reference's CTA scheduler
// (cuda/parallel/parallel_engine.h LBCTA :849-879).
// ===========================================================================

constexpr uint64_t kSmallDeg = 64;
constexpr uint64_t kMidDeg = 16384;

__device__ __forceinline__ bool row_has_edges(
    const uint64_t* __restrict__ off, const uint64_t* __restrict__ out_off,
    uint32_t r) {
  return off[r + 1] != off[r] || out_off[r + 1] != out_off[r];
}

// Pull-degree tiers (lists small/mid/large). Rows with no pull edge go into
// no list. Those that have no out-edge either (out_off == off for undirected
// graphs) are isolated and only counted: bin 3 for real rows, bin 4 for
// padding rows >= owned_real.
struct PullDegTiers {
  static constexpr int kLists = 3, kBins = 5;
  const uint64_t* __restrict__ off;
  const uint64_t* __restrict__ out_off;
  uint32_t owned_real;
  __device__ __forceinline__ int operator()(uint32_t r) const {
    uint64_t deg = off[r + 1] - off[r];
    if (deg) return deg < kSmallDeg ? 0 : (deg < kMidDeg ? 1 : 2);
    if (out_off[r + 1] == out_off[r]) return r < owned_real ? 3 : 4;
    return -1;
  }
};

// One bitmap word per thread: bit r%32 of word r/32 is set when owned row r
// has an edge. No atomics; compacted into rows_active (ascending).
__global__ void active_rows_bitmap_kernel(
    const uint64_t* __restrict__ off, const uint64_t* __restrict__ out_off,
    uint32_t owned, uint32_t* __restrict__ words, size_t nwords) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t w = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       w < nwords; w += stride) {
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
      uint64_t r = (static_cast<uint64_t>(w) << 5) + b;
      if (r < owned && row_has_edges(off, out_off, static_cast<uint32_t>(r)))
        bits |= 1u << b;
    }
    words[w] = bits;
  }
}

// degrees of a row list (hub work-list build)
__global__ void gather_row_deg_kernel(const uint64_t* __restrict__ off,
                                      const uint32_t* __restrict__ rows,
                                      uint64_t nrows,
                                      uint64_t* __restrict__ deg) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride)
    deg[i] = off[rows[i] + 1] - off[rows[i]];
}

// PageRank epilogue of the fused path: every owned row outside rows_active
// (isolated, padding included as before) takes the last iteration's base.
// Tests the row's bit in the active-row bitmap that the buckets keep
// (DeviceGraph::active_bm) instead of keeping a list of the isolated rows
// (296M entries at the benchmark shape) or reading two offsets per row.
__global__ void pr_fill_isolated_kernel(
    const uint32_t* __restrict__ active_bm, uint32_t owned, uint32_t v_begin,
    const double* __restrict__ last_base, double* __restrict__ rank) {
  const double base = *last_base;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       r < owned; r += stride)
    if (!((active_bm[r >> 5] >> (r & 31)) & 1u)) rank[v_begin + r] = base;
}

// Phase-split pulls (multi-GPU compute/comm overlap): the per-row
// adjacency is sorted ascending, so the owned dst range [lo,hi) is one
// contiguous span found by two binary searches. PHASE 0 = whole row
// (single-GPU / no overlap); PHASE 1 = owned span only, overwrite acc
// (runs WHILE the mirror exchange moves remote contribs on the comm
// stream); PHASE 2 = remaining spans, accumulate into acc.
__device__ __forceinline__ uint64_t lb_u32(const uint32_t* __restrict__ a,
                                           uint64_t lo, uint64_t hi,
                                           uint32_t key) {
  while (lo < hi) {
    uint64_t m = (lo + hi) >> 1;
    if (a[m] < key) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// maps a phase to an iteration domain over row [b,e): phase 1 iterates
// [L,R); phase 2 iterates [b,L) ++ [R,e) via a folded index.
struct PrSpan {
  uint64_t base1, n1, base2, n2;
  __device__ __forceinline__ uint64_t map(uint64_t k) const {
    return k < n1 ? base1 + k : base2 + (k - n1);
  }
  __device__ __forceinline__ uint64_t n() const { return n1 + n2; }
};

template <int PHASE>
__device__ __forceinline__ PrSpan pr_span(const uint32_t* __restrict__ dst,
                                          uint64_t b, uint64_t e,
                                          uint32_t lo, uint32_t hi) {
  if (PHASE == 0) return {b, e - b, 0, 0};
  uint64_t L = lb_u32(dst, b, e, lo), R = lb_u32(dst, b, e, hi);
  if (PHASE == 1) return {L, R - L, 0, 0};
  return {b, L - b, R, e - R};
}

// Edge-parallel small-row pull (CM idiom): thread-per-row streaming left
// each lane walking its own row — scattered 64B lines per 4B edge read.
// A block stages 256 short rows' spans in LDS, prefix-sums their
// lengths, then sweeps the chunk's edges with CONSECUTIVE lanes on
// consecutive edge slots (coalesced dst/contrib streams), wave-segmented
// sums per row and LDS fp64 accumulation at run tails.
// EPI 1, 2 (PHASE 0 only): the thread that would store the row's sum applies
// it instead (pr_row_done); the row length it staged is the row's degree.
template <int PHASE, int EPI = 0>
__global__ void pr_pull_small_cm_kernel(
    const uint64_t* __restrict__ off, const uint32_t* __restrict__ dst,
    const float* __restrict__ contrib, const uint32_t* __restrict__ rows,
    uint64_t nrows, uint32_t v_begin, uint32_t lo, uint32_t hi,
    double* __restrict__ acc, PrEpilogue ep) {
  static_assert(EPI == 0 || PHASE == 0, "epilogues need the whole row");
  __shared__ uint64_t s_b1[kBlock], s_b2[kBlock];
  __shared__ uint32_t s_n1[kBlock], s_pref[kBlock + 1];
  __shared__ double s_acc[kBlock];
  const int lane = threadIdx.x & 63;
  double ep_base = 0.0;
  if constexpr (EPI != 0) ep_base = *ep.base;
  for (uint64_t chunk = static_cast<uint64_t>(blockIdx.x) * kBlock;
       chunk < nrows;
       chunk += static_cast<uint64_t>(gridDim.x) * kBlock) {
    uint64_t i = chunk + threadIdx.x;
    uint32_t n = 0;
    if (i < nrows) {
      uint32_t r = rows[i];
      PrSpan sp = pr_span<PHASE>(dst, off[r], off[r + 1], lo, hi);
      s_b1[threadIdx.x] = sp.base1;
      s_n1[threadIdx.x] = static_cast<uint32_t>(sp.n1);
      s_b2[threadIdx.x] = sp.base2;
      n = static_cast<uint32_t>(sp.n());
    }
    s_acc[threadIdx.x] = 0.0;
    s_pref[threadIdx.x] = n;
    __syncthreads();
    // block-exclusive scan of the 256 lengths (Hillis-Steele in LDS)
    for (int d = 1; d < kBlock; d <<= 1) {
      uint32_t v = s_pref[threadIdx.x];
      uint32_t up = threadIdx.x >= d ? s_pref[threadIdx.x - d] : 0;
      __syncthreads();
      s_pref[threadIdx.x] = v + up;
      __syncthreads();
    }
    uint32_t total = s_pref[kBlock - 1];
    // shift to exclusive
    uint32_t excl = threadIdx.x ? s_pref[threadIdx.x - 1] : 0;
    __syncthreads();
    s_pref[threadIdx.x] = excl;
    if (threadIdx.x == 0) s_pref[kBlock] = total;
    __syncthreads();
    for (uint32_t base = 0; base < total; base += kBlock) {
      uint32_t e = base + threadIdx.x;
      bool act = e < total;
      uint32_t owner = 0xFFFFFFFFu;
      double c = 0.0;
      if (act) {
        uint32_t a = 0, b = kBlock;  // last owner with pref <= e
        while (a + 1 < b) {
          uint32_t m = (a + b) >> 1;
          if (s_pref[m] <= e) a = m;
          else b = m;
        }
        owner = a;
        uint32_t k = e - s_pref[a];
        uint64_t idx = k < s_n1[a]
                           ? s_b1[a] + k
                           : s_b2[a] + (k - s_n1[a]);
        c = static_cast<double>(contrib[dst[idx]]);
      }
      // wave-segmented sum keyed by owner (runs are contiguous)
      uint32_t oprev = __shfl_up(owner, 1, 64);
      bool head = (lane == 0) || oprev != owner;
      unsigned long long hb = __ballot(head);
      unsigned long long mine =
          hb & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1));
      int seg = 63 - __clzll(mine);
      double sum = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        double up = __shfl_up(sum, d, 64);
        if (lane - d >= seg) sum += up;
      }
      bool tail = (lane == 63) || ((hb >> (lane + 1)) & 1ull);
      if (tail && act) atomicAdd(&s_acc[owner], sum);
    }
    __syncthreads();
    if (i < nrows) {
      uint32_t r = rows[i];
      if constexpr (EPI != 0)
        pr_row_done<EPI>(ep, ep_base, v_begin + r, s_acc[threadIdx.x], n);
      else if (PHASE == 2) acc[v_begin + r] += s_acc[threadIdx.x];
      else acc[v_begin + r] = s_acc[threadIdx.x];
    }
    __syncthreads();
  }
}

// thread per row
template <int PHASE>
__global__ void pr_pull_small_kernel(const uint64_t* __restrict__ off,
                                     const uint32_t* __restrict__ dst,
                                     const float* __restrict__ contrib,
                                     const uint32_t* __restrict__ rows,
                                     uint64_t nrows, uint32_t v_begin,
                                     uint32_t lo, uint32_t hi,
                                     double* __restrict__ acc) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint32_t r = rows[i];
    PrSpan sp = pr_span<PHASE>(dst, off[r], off[r + 1], lo, hi);
    double sum = 0;
    for (uint64_t k = 0; k < sp.n(); ++k) sum += contrib[dst[sp.map(k)]];
    if (PHASE == 2) acc[v_begin + r] += sum;
    else acc[v_begin + r] = sum;
  }
}

// wave per row (4 waves per 256-block)
template <int PHASE>
__global__ void pr_pull_mid_kernel(const uint64_t* __restrict__ off,
                                   const uint32_t* __restrict__ dst,
                                   const float* __restrict__ contrib,
                                   const uint32_t* __restrict__ rows,
                                   uint64_t nrows, uint32_t v_begin,
                                   uint32_t lo, uint32_t hi,
                                   double* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves_per_block = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * waves_per_block;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * waves_per_block + wid;
       i < nrows; i += wstride) {
    uint32_t r = rows[i];
    PrSpan sp = pr_span<PHASE>(dst, off[r], off[r + 1], lo, hi);
    double sum = 0;
    for (uint64_t k = lane; k < sp.n(); k += kWave)
      sum += contrib[dst[sp.map(k)]];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (lane == 0) {
      if (PHASE == 2) acc[v_begin + r] += sum;
      else acc[v_begin + r] = sum;
    }
  }
}

// Hub rows (>= kMidDeg arcs): block per (row, segment) item of kHubSeg
// arcs, so a 0.7M-arc row spreads over ~170 blocks instead of serialising
// one. Each item writes one fp64 partial; pr_hub_reduce_kernel folds a
// row's partials in a fixed order (no fp64 atomics: results stay
// run-to-run deterministic). Segments are cut over the PHASE's span, so
// items past its end write 0.
constexpr uint32_t kHubSeg = 4096;

template <int PHASE>
__global__ void pr_pull_large_kernel(const uint64_t* __restrict__ off,
                                     const uint32_t* __restrict__ dst,
                                     const float* __restrict__ contrib,
                                     const uint32_t* __restrict__ rows,
                                     const uint32_t* __restrict__ item_row,
                                     const uint32_t* __restrict__ item_seg,
                                     uint64_t nitems, uint32_t lo,
                                     uint32_t hi,
                                     double* __restrict__ part) {
  __shared__ double s_wave[kBlock / kWave];
  for (uint64_t i = blockIdx.x; i < nitems; i += gridDim.x) {
    uint32_t r = rows[item_row[i]];
    PrSpan sp = pr_span<PHASE>(dst, off[r], off[r + 1], lo, hi);
    uint64_t kb = static_cast<uint64_t>(item_seg[i]) * kHubSeg;
    uint64_t ke = kb + kHubSeg < sp.n() ? kb + kHubSeg : sp.n();
    double sum = 0;
    for (uint64_t k = kb + threadIdx.x; k < ke; k += blockDim.x)
      sum += contrib[dst[sp.map(k)]];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0;
#pragma unroll
      for (int w = 0; w < kBlock / kWave; ++w) t += s_wave[w];
      part[i] = t;
    }
    __syncthreads();
  }
}

// wave per hub row: lanes stride the row's partials, then a fixed shuffle
// tree; the same order on every run.
template <int PHASE>
__global__ void pr_hub_reduce_kernel(const uint32_t* __restrict__ rows,
                                     const uint32_t* __restrict__ row_first,
                                     uint64_t nrows,
                                     const double* __restrict__ part,
                                     uint32_t v_begin,
                                     double* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves_per_block = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * waves_per_block;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * waves_per_block + wid;
       j < nrows; j += wstride) {
    double sum = 0;
    for (uint32_t k = row_first[j] + lane; k < row_first[j + 1]; k += kWave)
      sum += part[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (lane == 0) {
      uint32_t r = rows[j];
      if (PHASE == 2) acc[v_begin + r] += sum;
      else acc[v_begin + r] = sum;
    }
  }
}

// ===========================================================================
// PageRank id-segment pull (mid and hub rows, single GPU, PHASE 0).
//
// The row pulls gather contrib[dst] over the whole id range from every
// workgroup, so each XCD's private 4 MiB L2 tries to hold the same hot ids.
// Here the ids are cut into kPrSegs contiguous segments (PrSegView in
// dev_graph.hpp) and a workgroup prefers the items of the slice that
// belongs to the XCD it runs on, so that slice's contribs are gathered
// through one L2 only. Which workgroup takes which item decides speed and
// nothing else: every (span, item) partial is a sum in a fixed order,
// written once, and pr_seg_reduce_kernel folds a row's partials in
// (segment, item) order.
// ===========================================================================

// One bitmap word per thread: the rows of the mid and hub tiers.
__global__ void pr_seg_rows_bitmap_kernel(const uint64_t* __restrict__ off,
                                          uint32_t owned,
                                          uint32_t* __restrict__ words,
                                          size_t nwords) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t w = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       w < nwords; w += stride) {
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
      uint64_t r = (static_cast<uint64_t>(w) << 5) + b;
      if (r < owned && off[r + 1] - off[r] >= kSmallDeg) bits |= 1u << b;
    }
    words[w] = bits;
  }
}

struct PrSegBounds {
  uint32_t b[kPrSegs + 1];
};

// Wave per row: lanes 0..kPrSegs search the row's sorted adjacency for the
// segment bounds; len[s * nrows + j] is the length of row j's span in
// segment s (segment-major). A span of 2^32 arcs or more raises *too_long.
__global__ void pr_seg_cut_kernel(const uint64_t* __restrict__ off,
                                  const uint32_t* __restrict__ dst,
                                  const uint32_t* __restrict__ rows,
                                  uint64_t nrows, PrSegBounds bnd,
                                  uint32_t* __restrict__ len,
                                  int* __restrict__ too_long) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves_per_block = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * waves_per_block;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * waves_per_block + wid;
       j < nrows; j += wstride) {
    const uint32_t r = rows[j];
    const uint64_t b = off[r], e = off[r + 1];
    unsigned long long cut = e;
    if (lane == 0) cut = b;
    else if (lane < kPrSegs) cut = lb_u32(dst, b, e, bnd.b[lane]);
    const unsigned long long next = __shfl_down(cut, 1, 64);
    if (lane < kPrSegs) {
      const uint64_t l = next - cut;
      if (l > 0xFFFFFFFFull) *too_long = 1;
      len[static_cast<uint64_t>(lane) * nrows + j] = static_cast<uint32_t>(l);
    }
  }
}

// flag[idx] (segment-major): the span is not empty. pieces[j * kPrSegs + s]
// (row-major): the items it crosses, i.e. the partials it owns.
__global__ void pr_seg_pieces_kernel(const uint32_t* __restrict__ len,
                                     const uint64_t* __restrict__ pref,
                                     uint64_t nrows, uint32_t item,
                                     uint32_t* __restrict__ flag,
                                     uint32_t* __restrict__ pieces) {
  const uint64_t n = nrows * kPrSegs;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                      threadIdx.x;
       idx < n; idx += stride) {
    const uint64_t s = idx / nrows, j = idx - s * nrows;
    const uint64_t l = len[idx];
    const uint64_t a = pref[idx] - pref[s * nrows];
    flag[idx] = l ? 1u : 0u;
    pieces[j * kPrSegs + s] =
        l ? static_cast<uint32_t>((a + l - 1) / item - a / item + 1) : 0u;
  }
}

__global__ void pr_seg_fill_kernel(
    const uint32_t* __restrict__ len, const uint64_t* __restrict__ pref,
    const uint64_t* __restrict__ sid, const uint64_t* __restrict__ pfirst,
    const uint64_t* __restrict__ off, const uint32_t* __restrict__ rows,
    uint64_t nrows, uint64_t* __restrict__ span_pref,
    uint64_t* __restrict__ span_base, uint32_t* __restrict__ span_row,
    uint32_t* __restrict__ span_slot, uint64_t* __restrict__ row_first) {
  const uint64_t n = nrows * kPrSegs;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                      threadIdx.x;
       idx < n; idx += stride) {
    const uint64_t s = idx / nrows, j = idx - s * nrows;
    if (s == 0) row_first[j] = pfirst[j * kPrSegs];
    if (!len[idx]) continue;
    const uint64_t k = sid[idx];
    uint64_t base = off[rows[j]];
    for (uint64_t p = 0; p < s; ++p) base += len[p * nrows + j];
    span_pref[k] = pref[idx];
    span_base[k] = base;
    span_row[k] = static_cast<uint32_t>(j);
    span_slot[k] = static_cast<uint32_t>(pfirst[j * kPrSegs + s]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    span_pref[sid[n]] = pref[n];
    row_first[nrows] = pfirst[n];
  }
}

// The XCD this wave runs on (hardware register XCC_ID, bits 3:0).
__device__ __forceinline__ uint32_t xcc_id() {
  constexpr int kHwRegXccId = 20;
  return __builtin_amdgcn_s_getreg(((4 - 1) << 11) | kHwRegXccId);
}

// One window of 64 consecutive arcs of a wave's quarter: sums each span's run
// in lane order, continues the run carried in from the window before, stores
// a run that ends inside the window to wacc[owner] and carries the last one.
__device__ __forceinline__ void pr_seg_scan_window(int lane, bool act,
                                                   int owner, double c,
                                                   double* wacc, double& carry,
                                                   int& carry_owner) {
  const int oprev = __shfl_up(owner, 1, 64);
  const bool head = (lane == 0) || oprev != owner;
  const unsigned long long hb = __ballot(head);
  const unsigned long long mine =
      hb & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1));
  const int seg = 63 - __clzll(mine);
  double sum = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    double up = __shfl_up(sum, d, 64);
    if (lane - d >= seg) sum += up;
  }
  // the run that opens the window continues the carried one, or the
  // carried one is complete
  if (carry_owner >= 0) {
    if (owner == carry_owner && seg == 0) sum = carry + sum;
    const int o0 = __shfl(owner, 0, 64);
    if (o0 != carry_owner && lane == 0) wacc[carry_owner] = carry;
  }
  const bool tail = (lane == 63) || ((hb >> (lane + 1)) & 1ull);
  if (tail && act && lane != 63) wacc[owner] = sum;
  carry = __shfl(sum, 63, 64);
  carry_owner = __shfl(owner, 63, 64);
}

constexpr int kPrSegBlocksPerCu = 8;

// Persistent: CUs x kPrSegBlocksPerCu workgroups, each taking items from
// per-segment counters (ctr, zeroed before every launch).
template <bool NT, int DEPTH>
__global__ void __launch_bounds__(kBlock)
pr_pull_seg_kernel(PrSegView v, const uint32_t* __restrict__ dst,
                   const float* __restrict__ contrib,
                   uint32_t* __restrict__ ctr, double* __restrict__ part) {
  __shared__ uint64_t s_off[kBlock + 1];  // arc prefix of the batch's spans
  __shared__ uint64_t s_base[kBlock];
  __shared__ uint32_t s_slot[kBlock];
  __shared__ double s_wacc[kBlock / kWave][kBlock];  // per wave, per span
  __shared__ uint32_t s_take, s_first;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const uint32_t x = xcc_id() % kPrSlices;
  // Queue order: this XCD's slice, the head, the tail, then the other
  // slices. The loop ends on every path: a workgroup walks the kPrSegs
  // queues once, in this order, and never goes back; a counter only grows,
  // and every add either hands out one of the segment's n_items items or
  // returns a value past them, which moves the workgroup on to the next
  // queue. So a workgroup makes at most (items it processes) + kPrSegs
  // adds, waits for no other workgroup, and leaves after the last queue.
  for (int qi = 0; qi < kPrSegs; ++qi) {
    const int s = qi == 0   ? 1 + static_cast<int>(x)
                  : qi == 1 ? 0
                  : qi == 2 ? kPrSegs - 1
                            : 1 + static_cast<int>((x + qi - 2) % kPrSlices);
    const uint32_t n_items = v.n_items[s];
    if (!n_items) continue;
    const uint64_t* __restrict__ pref = v.span_pref + v.span_first[s];
    const uint64_t* __restrict__ sbase = v.span_base + v.span_first[s];
    const uint32_t* __restrict__ sslot = v.span_slot + v.span_first[s];
    const uint32_t qn =
        static_cast<uint32_t>(v.span_first[s + 1] - v.span_first[s]);
    const uint64_t arc0 = v.arc_first[s], arc1 = v.arc_first[s + 1];
    for (;;) {
      if (tid == 0) s_take = atomicAdd(&ctr[s], 1u);
      __syncthreads();
      const uint32_t t = s_take;
      if (t >= n_items) {
        __syncthreads();  // s_take is rewritten for the next queue
        break;
      }
      const uint64_t tile_lo = arc0 + static_cast<uint64_t>(t) * v.item;
      const uint64_t tile_hi = tile_lo + v.item < arc1 ? tile_lo + v.item : arc1;
      if (tid < kWave) {
        uint32_t first = wave_owner_search(pref, qn, tile_lo, tid);
        if (tid == 0) s_first = first;
      }
      __syncthreads();
      uint32_t chunk = s_first;
      for (;;) {
        const int n = min(static_cast<uint32_t>(kBlock), qn - chunk);
        if (tid < n) {
          const uint64_t o = pref[chunk + tid];
          s_off[tid] = o;
          // spans at or past the item's end own none of its arcs
          if (o < tile_hi) {
            s_base[tid] = sbase[chunk + tid];
            s_slot[tid] = sslot[chunk + tid];
          }
        }
        if (tid == 0) s_off[n] = pref[chunk + n];
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) s_wacc[w][tid] = 0.0;
        __syncthreads();
        const uint64_t batch_end = s_off[n];
        const uint64_t e0 = s_off[0] > tile_lo ? s_off[0] : tile_lo;
        const uint64_t e1 = batch_end < tile_hi ? batch_end : tile_hi;
        // each wave sums one contiguous quarter of [e0, e1) in windows of 64
        // consecutive arcs; a span's run inside the quarter is summed in
        // lane order, carried from window to window, and stored once
        const uint64_t quarter =
            ((e1 - e0 + kBlock - 1) / kBlock) * kWave;
        const uint64_t ws = e0 + wid * quarter;
        const uint64_t we = ws + quarter < e1 ? ws + quarter : e1;
        int lo = 0;
        if (ws + lane < we) {
          int hi = n - 1;
          const uint64_t e = ws + lane;
          while (lo < hi) {
            int mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= e) lo = mid; else hi = mid - 1;
          }
        }
        double carry = 0.0;
        int carry_owner = -1;
        for (uint64_t g0 = ws; g0 < we; g0 += DEPTH * kWave) {
          // a group of DEPTH windows: every dst load, then every gather,
          // then the scans in window order (KERNELS.md "Arc depth")
          bool act[DEPTH];
          int owner[DEPTH];
          float cf[DEPTH];
          if constexpr (DEPTH == 1) {
            const uint64_t e = g0 + lane;
            act[0] = e < we;
            owner[0] = -1;
            cf[0] = 0.0f;
            if (act[0]) {
              while (lo + 1 < n && s_off[lo + 1] <= e) ++lo;
              owner[0] = lo;
              const uint64_t idx = s_base[lo] + (e - s_off[lo]);
              const uint32_t d = NT ? __builtin_nontemporal_load(dst + idx)
                                    : dst[idx];
              cf[0] = contrib[d];
            }
          } else {
            // a lane past the quarter's end loads arc 0 of the CSR, which
            // exists (the segment has an item), and drops the value: the
            // loads stay unconditional, so none waits for another
            uint64_t idx[DEPTH];
            uint32_t d[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
              const uint64_t e = g0 + j * kWave + lane;
              act[j] = e < we;
              owner[j] = -1;
              idx[j] = 0;
              if (act[j]) {
                while (lo + 1 < n && s_off[lo + 1] <= e) ++lo;
                owner[j] = lo;
                idx[j] = s_base[lo] + (e - s_off[lo]);
              }
            }
#pragma unroll
            for (int j = 0; j < DEPTH; ++j)
              d[j] = NT ? __builtin_nontemporal_load(dst + idx[j])
                        : dst[idx[j]];
            // left alone, the scheduler interleaves the rounds again to
            // save registers (load, wait, load, wait): fence them
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) cf[j] = contrib[d[j]];
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int j = 0; j < DEPTH; ++j) {
            // the quarter may end inside the group (the same for all lanes)
            if (DEPTH > 1 && g0 + j * kWave >= we) break;
            const double c = act[j] ? static_cast<double>(cf[j]) : 0.0;
            pr_seg_scan_window(lane, act[j], owner[j], c, s_wacc[wid], carry,
                               carry_owner);
          }
        }
        if (carry_owner >= 0 && lane == 0) s_wacc[wid][carry_owner] = carry;
        __syncthreads();
        if (tid < n && s_off[tid] < e1 && s_off[tid + 1] > e0) {
          double total = 0.0;
#pragma unroll
          for (int w = 0; w < kBlock / kWave; ++w) total += s_wacc[w][tid];
          const uint64_t first_item = (s_off[tid] - arc0) / v.item;
          part[s_slot[tid] + (t - first_item)] = total;
        }
        __syncthreads();
        if (batch_end >= tile_hi || chunk + n >= qn) break;
        chunk += n;
      }
    }
  }
}

// Folds a row's partials in (segment, item) order: a lane per row, and the
// whole wave, in a fixed tree, for a row with more than 64 of them.
// EPI 1, 2: the lane that would store the row's sum applies it instead
// (pr_row_done), with the row's degree from row_deg.
template <int EPI = 0>
__global__ void pr_seg_reduce_kernel(const uint32_t* __restrict__ rows,
                                     const uint64_t* __restrict__ row_first,
                                     uint64_t nrows,
                                     const double* __restrict__ part,
                                     uint32_t v_begin,
                                     double* __restrict__ acc,
                                     const uint32_t* __restrict__ row_deg,
                                     PrEpilogue ep) {
  const int lane = threadIdx.x & 63;
  double ep_base = 0.0;
  if constexpr (EPI != 0) ep_base = *ep.base;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                     (threadIdx.x - lane);
       j0 < nrows; j0 += stride) {
    const uint64_t j = j0 + lane;
    unsigned long long b = 0, e = 0;
    if (j < nrows) {
      b = row_first[j];
      e = row_first[j + 1];
    }
    const bool wide = e - b > kWave;
    double sum = 0.0;
    if (!wide)
      for (uint64_t k = b; k < e; ++k) sum += part[k];
    unsigned long long todo = __ballot(wide);
    while (todo) {
      const int l = __ffsll(todo) - 1;
      todo &= todo - 1;
      const unsigned long long bb = __shfl(b, l, 64), ee = __shfl(e, l, 64);
      double t = 0.0;
      for (uint64_t k = bb + lane; k < ee; k += kWave) t += part[k];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d, 64);
      t = __shfl(t, 0, 64);
      if (lane == l) sum = t;
    }
    if (j < nrows) {
      if constexpr (EPI != 0)
        pr_row_done<EPI>(ep, ep_base, v_begin + rows[j], sum, row_deg[j]);
      else
        acc[v_begin + rows[j]] = sum;
    }
  }
}

// The degrees of the id-segment rows, for the reduce's epilogue. A row of
// 2^32 arcs or more raises *too_long.
__global__ void pr_seg_row_deg_kernel(const uint64_t* __restrict__ off,
                                      const uint32_t* __restrict__ rows,
                                      uint64_t nrows,
                                      uint32_t* __restrict__ deg,
                                      int* __restrict__ too_long) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       j < nrows; j += stride) {
    const uint64_t d = off[rows[j] + 1] - off[rows[j]];
    if (d > 0xFFFFFFFFull) *too_long = 1;
    deg[j] = static_cast<uint32_t>(d);
  }
}

// ===========================================================================
// PageRank tiled pull. The row-major pull gathers contrib[dst] across the
// whole vertex range: at datagen-9_0 scale every 4-byte gather fetches a
// distinct 64-byte line (~6% line use, r01 PMC: 2.3 TB/s fetch, >80%
// latency stall). Regrouping edges by DST TILE (4096 vertices = 16 KB of
// contribs) makes consecutive gathers hit the same L2-resident window, so
// per-iteration traffic drops to ~(8 B/edge edge stream + one pass over
// contrib + L2-resident acc atomics). Rows' dst lists are sorted, so each
// row contributes contiguous per-tile runs; runs are placed contiguously
// inside their tile bucket (order across rows is irrelevant — each run
// has constant src, and a wave-segmented sum emits one fp64 atomic per
// run per 64-edge window). Built once per graph, cached in HBM3E
// (8 B/stored edge).
// ===========================================================================

constexpr int kPrTileBits = 12;  // 4096 vertices/tile: 16 KB fp32 window

// count (out==nullptr) or place (out!=nullptr) per-row tile runs.
// thread-per-row variant for short rows.
__global__ void pr_tile_runs_small_kernel(
    const uint64_t* __restrict__ off, const uint32_t* __restrict__ dst,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint32_t r = rows[i];
    uint64_t b = off[r], e = off[r + 1];
    uint64_t src64 = static_cast<uint64_t>(v_begin + r) << 32;
    uint64_t k = b;
    while (k < e) {
      uint32_t t = dst[k] >> kPrTileBits;
      uint64_t j = k + 1;
      while (j < e && (dst[j] >> kPrTileBits) == t) ++j;
      unsigned long long pos = atomicAdd(&cnt[t], j - k);
      if (out)
        for (uint64_t q = k; q < j; ++q)
          out[pos + (q - k)] = src64 | dst[q];
      k = j;
    }
  }
}

// wave-per-row variant: lanes stride the row; run boundaries via ballot.
__global__ void pr_tile_runs_wave_kernel(
    const uint64_t* __restrict__ off, const uint32_t* __restrict__ dst,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < nrows;
       i += wstride) {
    uint32_t r = rows[i];
    uint64_t b = off[r], e = off[r + 1];
    uint64_t src64 = static_cast<uint64_t>(v_begin + r) << 32;
    for (uint64_t base = b; base < e; base += kWave) {
      uint64_t k = base + lane;
      bool act = k < e;
      uint32_t d = act ? dst[k] : 0xFFFFFFFFu;
      uint32_t t = d >> kPrTileBits;
      // head: first lane of window, or tile differs from previous lane's
      uint32_t tprev = __shfl_up(t, 1, 64);
      bool head = act && (lane == 0 || tprev != t ||
                          (base + lane - 1) < b);
      // window runs may continue the previous window's run: lane0 head
      // still claims fresh space — runs split at window boundaries,
      // which only adds an extra atomic, not an error
      unsigned long long hb = __ballot(head);
      unsigned long long pos = 0;
      if (head && act) {
        // run length = next head (or window end / row end) - k
        unsigned long long later = hb >> 1 >> lane;  // heads after me
        int next = later ? lane + 1 + __ffsll(later) - 1 : 64;
        uint64_t rend = base + next;
        if (rend > e) rend = e;
        pos = atomicAdd(&cnt[t], rend - k);
      }
      if (out && act) {
        // my position: broadcast pos from my run's head lane
        unsigned long long mine =
            hb & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1));
        int myhead = 63 - __clzll(mine);
        unsigned long long hpos =
            __shfl(pos, myhead, 64);
        out[hpos + (lane - myhead)] = src64 | d;
      }
    }
  }
}

// one pass over the tiled edge stream: gather contrib from the L2-hot
// window, wave-segmented sum per constant-src run, fp64 atomic per run.
__global__ void pr_tiled_pull_kernel(
    const unsigned long long* __restrict__ tiles, uint64_t lo, uint64_t hi,
    const float* __restrict__ contrib, double* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  uint64_t n = hi - lo;
  if (!n) return;
  // contiguous chunk per wave (keeps each wave inside one tile window)
  uint64_t waves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) / kWave;
  uint64_t wid = (static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                  threadIdx.x) / kWave;
  uint64_t chunk = (n + waves - 1) / waves;
  uint64_t wb = lo + wid * chunk;
  uint64_t we = wb + chunk < hi ? wb + chunk : hi;
  for (uint64_t base = wb; base < we; base += kWave) {
    uint64_t k = base + lane;
    bool act = k < we;
    unsigned long long rec = act ? tiles[k] : ~0ull;
    uint32_t srcv = static_cast<uint32_t>(rec >> 32);
    double c = act ? static_cast<double>(contrib[static_cast<uint32_t>(rec)])
                   : 0.0;
    uint32_t sprev = __shfl_up(srcv, 1, 64);
    bool head = (lane == 0) || sprev != srcv;
    unsigned long long hb = __ballot(head);
    // segment start = highest head lane <= me
    unsigned long long mine =
        hb & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1));
    int seg = 63 - __clzll(mine);
    double sum = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      double up = __shfl_up(sum, d, 64);
      if (lane - d >= seg) sum += up;
    }
    bool tail = (lane == 63) || ((hb >> (lane + 1)) & 1ull);
    if (tail && act && srcv != 0xFFFFFFFFu) atomicAdd(&acc[srcv], sum);
  }
}


// ---------------------------------------------------------------------------
// Direction-optimizing BFS pull kernels (reference cuda/bfs/bfs.h :206-260):
// sweep unvisited owned rows looking for a parent at the current level.
// No atomics, early exit; reuses the degree buckets.
// ---------------------------------------------------------------------------
__global__ void bfs_pull_small_kernel(const uint64_t* __restrict__ off,
                                      const uint32_t* __restrict__ dst,
                                      const uint32_t* __restrict__ rows,
                                      uint64_t nrows, uint32_t v_begin,
                                      uint32_t* __restrict__ depth,
                                      uint32_t level, DevBitmap next_bm) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint32_t r = rows[i];
    uint32_t v = v_begin + r;
    if (depth[v] != 0xFFFFFFFFu) continue;
    uint64_t b = off[r], e = off[r + 1];
    for (uint64_t k = b; k < e; ++k) {
      if (depth[dst[k]] == level) {
        depth[v] = level + 1;
        next_bm.set_once(r);
        break;
      }
    }
  }
}

__global__ void bfs_pull_mid_kernel(const uint64_t* __restrict__ off,
                                    const uint32_t* __restrict__ dst,
                                    const uint32_t* __restrict__ rows,
                                    uint64_t nrows, uint32_t v_begin,
                                    uint32_t* __restrict__ depth,
                                    uint32_t level, DevBitmap next_bm) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < nrows;
       i += wstride) {
    uint32_t r = rows[i];
    uint32_t v = v_begin + r;
    if (depth[v] != 0xFFFFFFFFu) continue;
    uint64_t b = off[r], e = off[r + 1];
    bool found = false;
    for (uint64_t kb = b; kb < e; kb += kWave) {
      uint64_t k = kb + lane;
      bool mine = k < e && depth[dst[k]] == level;
      if (__any(mine)) {
        found = true;
        break;
      }
    }
    if (found && lane == 0) {
      depth[v] = level + 1;
      next_bm.set_once(r);
    }
  }
}

__global__ void bfs_pull_large_kernel(const uint64_t* __restrict__ off,
                                      const uint32_t* __restrict__ dst,
                                      const uint32_t* __restrict__ rows,
                                      uint64_t nrows, uint32_t v_begin,
                                      uint32_t* __restrict__ depth,
                                      uint32_t level, DevBitmap next_bm) {
  __shared__ int s_found;
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    uint32_t v = v_begin + r;
    if (depth[v] != 0xFFFFFFFFu) continue;
    uint64_t b = off[r], e = off[r + 1];
    if (threadIdx.x == 0) s_found = 0;
    __syncthreads();
    for (uint64_t kb = b; kb < e; kb += blockDim.x) {
      uint64_t k = kb + threadIdx.x;
      if (k < e && depth[dst[k]] == level) s_found = 1;
      __syncthreads();
      if (s_found) break;
      __syncthreads();
    }
    if (threadIdx.x == 0 && s_found) {
      depth[v] = level + 1;
      next_bm.set_once(r);
    }
    __syncthreads();
  }
}

// ===========================================================================
// GpuContext implementation
// ===========================================================================

// ===========================================================================
// Device data plane. Production path: RCCL over xGMI, one rank per GPU
// (reference gpu_message_manager.h NCCL ring, RCCL is the MI355X drop-in).
// Validation path: TCP-staged collectives for when several ranks share one
// device (RCCL refuses duplicate GPUs) — selected by GRAPEHIP_DATAPLANE=tcp
// or auto-detected at init. Both paths drive the IDENTICAL call sites, so
// the world-N halo/allgather/reduce-scatter logic is exercised end-to-end
// on a one-GPU lease before an 8-GPU node ever sees it.
// ===========================================================================
struct DevComm {
  ncclComm_t nccl = nullptr;
  TcpComm* tcp = nullptr;
  int rank = 0, world = 1;
  bool use_tcp = false;
  // per-rank data-plane byte accounting (this rank's sends), split into
  // point-to-point (halo/mirror/row-fetch) and collective traffic —
  // read back per app run so comm volume vs boundary size is observable
  uint64_t bytes_p2p = 0, bytes_coll = 0;

  bool active() const { return world > 1; }

  // --- tcp staging helpers (host bounce; correctness path, not perf) ------
  std::string stage_out(const void* dev, size_t n, hipStream_t s) const {
    std::string h(n, '\0');
    HIP_CHECK(hipStreamSynchronize(s));
    if (n) HIP_CHECK(hipMemcpy(h.data(), dev, n, hipMemcpyDeviceToHost));
    return h;
  }
  void stage_in(void* dev, const void* host, size_t n) const {
    if (n) HIP_CHECK(hipMemcpy(dev, host, n, hipMemcpyHostToDevice));
  }

  // In-place allgather of 4-byte slices: buf[rank*slice .. ) is this rank's
  // contribution; on return buf[0 .. world*slice) holds every rank's.
  void allgather32(void* buf, uint64_t slice, bool fp, hipStream_t s) {
    if (!active()) return;
    bytes_coll += slice * 4;
    if (!use_tcp) {
      NCCL_CHECK(ncclAllGather(
          static_cast<char*>(buf) + static_cast<uint64_t>(rank) * slice * 4,
          buf, slice, fp ? ncclFloat : ncclUint32, nccl, s));
      return;
    }
    std::string mine = stage_out(
        static_cast<char*>(buf) + static_cast<uint64_t>(rank) * slice * 4,
        slice * 4, s);
    std::vector<char> all(static_cast<size_t>(world) * slice * 4);
    tcp->allgather(mine.data(), slice * 4, all.data());
    stage_in(buf, all.data(), all.size());
  }

  // In-place reduce-scatter (sum, f64): buf holds world*slice doubles; on
  // return buf[rank*slice ..) = elementwise sum of every rank's slice.
  void reduce_scatter_sum_f64(double* buf, uint64_t slice, hipStream_t s) {
    if (!active()) return;
    bytes_coll += static_cast<uint64_t>(world) * slice * 8;
    if (!use_tcp) {
      NCCL_CHECK(ncclReduceScatter(
          buf, buf + static_cast<uint64_t>(rank) * slice, slice, ncclDouble,
          ncclSum, nccl, s));
      return;
    }
    std::string full =
        stage_out(buf, static_cast<size_t>(world) * slice * 8, s);
    const double* h = reinterpret_cast<const double*>(full.data());
    std::vector<std::string> send(world);
    for (int p = 0; p < world; ++p)
      send[p].assign(
          reinterpret_cast<const char*>(h + static_cast<uint64_t>(p) * slice),
          slice * 8);
    auto recv = tcp->exchange_all(send);
    std::vector<double> acc(slice, 0.0);
    for (int p = 0; p < world; ++p) {
      const double* rp = reinterpret_cast<const double*>(recv[p].data());
      for (uint64_t i = 0; i < slice; ++i) acc[i] += rp[i];
    }
    stage_in(buf + static_cast<uint64_t>(rank) * slice, acc.data(),
             slice * 8);
  }

  void allreduce_min_u32(uint32_t* buf, uint64_t n, hipStream_t s) {
    if (!active()) return;
    bytes_coll += n * 4;
    if (!use_tcp) {
      NCCL_CHECK(
          ncclAllReduce(buf, buf, n, ncclUint32, ncclMin, nccl, s));
      return;
    }
    std::string mine = stage_out(buf, n * 4, s);
    std::vector<uint32_t> all(static_cast<size_t>(world) * n);
    tcp->allgather(mine.data(), n * 4, all.data());
    uint32_t* acc = reinterpret_cast<uint32_t*>(mine.data());
    for (int p = 0; p < world; ++p) {
      const uint32_t* rp = all.data() + static_cast<uint64_t>(p) * n;
      for (uint64_t i = 0; i < n; ++i)
        if (rp[i] < acc[i]) acc[i] = rp[i];
    }
    stage_in(buf, acc, n * 4);
  }

  void allreduce_sum_u64(unsigned long long* buf, uint64_t n,
                         hipStream_t s) {
    if (!active()) return;
    bytes_coll += n * 8;
    if (!use_tcp) {
      NCCL_CHECK(ncclAllReduce(buf, buf, n, ncclUint64, ncclSum, nccl, s));
      return;
    }
    std::string mine = stage_out(buf, n * 8, s);
    std::vector<unsigned long long> all(static_cast<size_t>(world) * n);
    tcp->allgather(mine.data(), n * 8, all.data());
    unsigned long long* acc =
        reinterpret_cast<unsigned long long*>(mine.data());
    for (uint64_t i = 0; i < n; ++i) acc[i] = 0;
    for (int p = 0; p < world; ++p) {
      const unsigned long long* rp =
          all.data() + static_cast<uint64_t>(p) * n;
      for (uint64_t i = 0; i < n; ++i) acc[i] += rp[i];
    }
    stage_in(buf, acc, n * 8);
  }

  // Pairwise variable-size exchange: send_off/recv_off are [world+1] byte
  // offsets into sendbuf/recvbuf; peer p receives this rank's region p.
  // Self region is handled by the caller (halo appends skip owned ids).
  void sendrecv(const uint8_t* sendbuf, const std::vector<uint64_t>& send_off,
                uint8_t* recvbuf, const std::vector<uint64_t>& recv_off,
                hipStream_t s) {
    if (!active()) return;
    for (int p = 0; p < world; ++p)
      if (p != rank) bytes_p2p += send_off[p + 1] - send_off[p];
    if (!use_tcp) {
      NCCL_CHECK(ncclGroupStart());
      for (int p = 0; p < world; ++p) {
        if (p == rank) continue;
        uint64_t to_p = send_off[p + 1] - send_off[p];
        uint64_t from_p = recv_off[p + 1] - recv_off[p];
        if (to_p)
          NCCL_CHECK(ncclSend(sendbuf + send_off[p], to_p, ncclChar, p,
                              nccl, s));
        if (from_p)
          NCCL_CHECK(ncclRecv(recvbuf + recv_off[p], from_p, ncclChar, p,
                              nccl, s));
      }
      NCCL_CHECK(ncclGroupEnd());
      return;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    std::vector<std::string> send(world);
    for (int p = 0; p < world; ++p) {
      if (p == rank) continue;
      uint64_t n = send_off[p + 1] - send_off[p];
      send[p] = stage_out(sendbuf + send_off[p], n, s);
    }
    auto recv = tcp->exchange_all(send);
    for (int p = 0; p < world; ++p) {
      if (p == rank) continue;
      uint64_t n = recv_off[p + 1] - recv_off[p];
      if (n != recv[p].size())
        throw std::runtime_error("sendrecv(tcp): size mismatch");
      stage_in(recvbuf + recv_off[p], recv[p].data(), n);
    }
  }

  // Ragged in-place allgather: rank f owns buf[region[f]*4 .. region[f+1]*4)
  // (u32 elements); every rank ends with all regions populated.
  void bcast_regions_u32(uint32_t* buf, const std::vector<uint64_t>& region,
                         hipStream_t s) {
    if (!active()) return;
    bytes_coll += (region[rank + 1] - region[rank]) * 4;
    if (!use_tcp) {
      NCCL_CHECK(ncclGroupStart());
      for (int f = 0; f < world; ++f) {
        uint64_t cnt_f = region[f + 1] - region[f];
        if (cnt_f)
          NCCL_CHECK(ncclBroadcast(buf + region[f], buf + region[f], cnt_f,
                                   ncclUint32, f, nccl, s));
      }
      NCCL_CHECK(ncclGroupEnd());
      return;
    }
    uint64_t mine_n = region[rank + 1] - region[rank];
    std::string mine = stage_out(buf + region[rank], mine_n * 4, s);
    std::vector<std::string> send(world, mine);
    auto recv = tcp->exchange_all(send);
    for (int f = 0; f < world; ++f) {
      if (f == rank) continue;
      uint64_t n = region[f + 1] - region[f];
      if (n * 4 != recv[f].size())
        throw std::runtime_error("bcast_regions(tcp): size mismatch");
      stage_in(buf + region[f], recv[f].data(), n * 4);
    }
  }
};

enum LbKind { kLbCm = 0, kLbWm, kLbStrict, kLbNone, kLbCount };

struct GpuContext::Impl {
  DevComm dc;
  Stream compute;
  Stream comm_stream;
  Event ev_pack;   // compute -> comm ordering for the halo exchange
  Event ev_comm;   // comm -> compute ordering (recv payload ready)
  Event ev_scal;   // pinned-scalar D2H landed (host folds while GPU works)
  double* h_scal = nullptr;  // 2 pinned doubles: [0] local out, [1] global in
  Impl() { HIP_CHECK(hipHostMalloc(&h_scal, 2 * sizeof(double))); }
  ~Impl() {
    if (h_scal) (void)hipHostFree(h_scal);
  }
  ScanTemp scan;
  // halo scratch (sized on first use)
  DeviceBuffer<uint32_t> halo_idx;
  DeviceBuffer<unsigned long long> halo_cnt;
  DeviceBuffer<uint32_t> halo_bm;
  DeviceBuffer<uint8_t> sendbuf, recvbuf;
  // frontier scratch
  DeviceBuffer<uint32_t> frontier_deg;
  DeviceBuffer<uint64_t> frontier_off;
  // traversal workspace of bfs()/sssp(): grows, never shrinks, freed with
  // the context. Both apps share it and initialise what they use inside
  // their timed region; a call on a smaller graph uses a prefix.
  DeviceBuffer<uint32_t> trav_state;   // BFS depth / SSSP distance bits
  DeviceBuffer<uint32_t> trav_q[4];    // [0] BFS queue; SSSP near/far pairs
  DeviceBuffer<uint32_t> trav_near_bm, trav_far_bm;
  DeviceBuffer<unsigned long long> trav_fcnt;  // SSSP far queue counters
  DeviceBuffer<uint32_t> trav_fdeg;    // frontier degrees (separate from the
  DeviceBuffer<uint64_t> trav_foff;    //  compaction scratch above)
  // bc() fp64 workspace, grow-only like the above: path counts and
  // dependency sums by global vid, push coefficients by owned row. bc()
  // also uses trav_state (depth), trav_q[0] (the level-order array),
  // trav_near_bm and trav_fdeg/trav_foff.
  DeviceBuffer<double> bc_sigma, bc_acc, bc_coef;
  double t_exchange = 0;
  // host-side count of frontier expansions dispatched per scheduler
  // (launch_expand only, a frontier without an arc included; test hook,
  // see debug_expand_counts)
  uint64_t expand_counts[kLbCount] = {0, 0, 0, 0};
  // pagerank() calls through the id-segment pull [0] and the row-tier
  // pulls [1] (test hook, see debug_pr_path)
  uint64_t pr_path_counts[2] = {0, 0};
  // pagerank() calls on the epilogue path [0], their iterations replayed
  // from a captured hipGraph [1] (test hook, see debug_pr_epilogue)
  uint64_t pr_epi_counts[2] = {0, 0};
  // device kclique() calls so far, and the rows of the last one in the
  // wave, block and global tiers (test hook, see debug_kclique)
  uint64_t kclique_calls = 0;
  uint64_t kclique_rows[3] = {0, 0, 0};
  // sample() workspace, grow-only like the traversal buffers: the two
  // walker queues and the per-peer send regions (8 B per walk each, the
  // regions per peer), the path table (4 B per walk and hop), the counters
  // and the start / owned-walk / result staging
  DeviceBuffer<unsigned long long> sample_q[2], sample_peer, sample_cnt;
  DeviceBuffer<uint32_t> sample_paths, sample_starts, sample_own, sample_out;
  GpuContext::SampleDebug sample_dbg;  // test hook, see debug_sample
  int num_cus = 256;  // set by the GpuContext constructor
};

namespace {

DevGraphView make_view(const DeviceGraph& g, int rank, int world) {
  DevGraphView v{};
  v.nv_global = g.nv_global;
  v.v_begin = g.v_begin;
  v.v_end = g.v_end;
  v.slice = g.seg_host.size() > 1 ? (g.seg_host[1] - g.seg_host[0])
                                  : g.nv_global;
  if (v.slice == 0) v.slice = 1;
  v.rank = rank;
  v.world = world;
  v.oe_off = g.oe_off.data();
  v.oe_dst = g.oe_dst.data();
  v.oe_w = g.weighted ? g.oe_w.data() : nullptr;
  v.ie_off = g.has_in ? g.ie_off.data() : nullptr;
  v.ie_dst = g.has_in ? g.ie_dst.data() : nullptr;
  v.ie_w = (g.has_in && g.weighted) ? g.ie_w.data() : nullptr;
  v.seg = g.seg.data();
  return v;
}

uint32_t padded_nv(const DeviceGraph& g, int world) {
  uint32_t slice = g.seg_host.size() > 1 ? (g.seg_host[1] - g.seg_host[0])
                                         : g.nv_global;
  uint64_t pad = static_cast<uint64_t>(slice) * world;
  return static_cast<uint32_t>(pad > g.nv_global ? pad : g.nv_global);
}

// grow-only resize: contents are not kept
template <typename T>
void grow(DeviceBuffer<T>& b, size_t n) {
  if (b.size() < n) b.resize(n);
}

double wall_s() {
  return std::chrono::duration<double>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// The timed region of an app run. Opens with control-plane barrier, device
// sync, clock; finish() closes with device sync, barrier, clock, and takes
// the slowest rank's time. Whatever the app enqueues between the two is
// what `seconds` measures.
struct RunBracket {
  GpuContext::Impl& I;
  TcpComm* comm;
  double t0;
  uint64_t b_p2p0, b_coll0;
  RunBracket(GpuContext::Impl& impl, TcpComm* c) : I(impl), comm(c) {
    if (comm) comm->barrier();
    HIP_CHECK(hipDeviceSynchronize());
    t0 = wall_s();
    b_p2p0 = I.dc.bytes_p2p, b_coll0 = I.dc.bytes_coll;
  }
  double elapsed_ms() const { return (wall_s() - t0) * 1e3; }
  GpuRunResult finish(int rounds, uint64_t traversed_edges) const {
    HIP_CHECK(hipDeviceSynchronize());
    if (comm) comm->barrier();
    double t1 = wall_s();
    GpuRunResult res;
    res.bytes_p2p = I.dc.bytes_p2p - b_p2p0;
    res.bytes_coll = I.dc.bytes_coll - b_coll0;
    res.rounds = rounds;
    res.seconds = comm ? comm->allreduce_max_double(t1 - t0) : (t1 - t0);
    res.traversed_edges = traversed_edges;
    return res;
  }
};

// Sorts the keys of every row of `off` (rows_n + 1 offsets into the codec's
// arrays) ascending, on stream s. Reads the two tier counts back, so it
// syncs s once; the sort kernels themselves are left in flight.
template <typename Codec>
void segmented_sort_rows(const uint64_t* off, uint32_t rows_n, Codec codec,
                         hipStream_t s, ScanTemp& scan) {
  using Key = typename Codec::Key;
  DeviceBuffer<uint32_t> lds_rows, big_rows;
  auto h = partition_rows(SortLenTiers{off}, rows_n, {&lds_rows, &big_rows},
                          s);
  const uint64_t n_lds = h[0], n_big = h[1];
  if (n_lds)
    seg_sort_lds_kernel<<<std::min<uint64_t>(n_lds, kMaxGrid), kBlock, 0,
                          s>>>(off, codec, lds_rows.data(), n_lds);
  if (n_big) {
    const int grid = static_cast<int>(std::min<uint64_t>(n_big, kMaxGrid));
    DeviceBuffer<uint32_t> caps(n_big);
    DeviceBuffer<uint64_t> pad_off(n_big + 1);
    seg_bigcap_kernel<<<grid_for(n_big), kBlock, 0, s>>>(
        off, big_rows.data(), n_big, caps.data());
    uint64_t pad_total =
        exclusive_scan(caps.data(), pad_off.data(), n_big, s, scan);
    DeviceBuffer<Key> scratch(pad_total);
    seg_bigpad_kernel<<<grid, kBlock, 0, s>>>(
        off, codec, big_rows.data(), n_big, pad_off.data(), scratch.data());
    seg_bigsort_kernel<<<grid, kBlock, 0, s>>>(pad_off.data(), n_big,
                                               scratch.data());
    seg_bigunpad_kernel<<<grid, kBlock, 0, s>>>(
        off, codec, big_rows.data(), n_big, pad_off.data(), scratch.data());
  }
}

}  // namespace

DeviceGraph::~DeviceGraph() {
  if (pr_graph_exec)
    (void)hipGraphExecDestroy(
        reinterpret_cast<hipGraphExec_t>(pr_graph_exec));
  for (void* e : pr_epi_exec)
    if (e) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(e));
}

GpuContext::GpuContext(TcpComm* comm, int rank, int world)
    : comm_(comm), rank_(rank), world_(world) {
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  if (ndev == 0) throw std::runtime_error("no HIP devices visible");
  const char* lr = std::getenv("LOCAL_RANK");
  dev_ = lr ? (std::atoi(lr) % ndev) : (rank % ndev);
  HIP_CHECK(hipSetDevice(dev_));
  impl_ = std::make_unique<Impl>();
  HIP_CHECK(hipDeviceGetAttribute(&impl_->num_cus,
                                  hipDeviceAttributeMultiprocessorCount,
                                  dev_));
  DevComm& dc = impl_->dc;
  dc.tcp = comm;
  dc.rank = rank;
  dc.world = world;
  if (world > 1) {
    // data-plane pick: RCCL needs one distinct GPU per rank; ranks that
    // share a device (world-N validation on a 1-GPU lease) stage through
    // the TCP control plane instead. Same call sites either way.
    const char* dp = std::getenv("GRAPEHIP_DATAPLANE");
    if (dp && std::string(dp) == "tcp") {
      dc.use_tcp = true;
    } else if (dp && std::string(dp) == "rccl") {
      dc.use_tcp = false;
    } else {
      std::vector<int> devs(world);
      comm->allgather(&dev_, sizeof(int), devs.data());
      std::sort(devs.begin(), devs.end());
      dc.use_tcp = std::adjacent_find(devs.begin(), devs.end()) !=
                   devs.end();
    }
    if (!dc.use_tcp) {
      ncclUniqueId id;
      if (rank == 0) NCCL_CHECK(ncclGetUniqueId(&id));
      comm->bcast(&id, sizeof(id), 0);
      NCCL_CHECK(ncclCommInitRank(&dc.nccl, world, id, rank));
      // warm up the xGMI links (reference WarmupNccl, dev_utils.h:894)
      DeviceBuffer<float> dummy(world * 256);
      NCCL_CHECK(ncclAllReduce(dummy.data(), dummy.data(), 256, ncclFloat,
                               ncclSum, dc.nccl, impl_->compute));
      impl_->compute.sync();
    } else if (getenv("GRAPEHIP_DEBUG")) {
      fprintf(stderr, "[dc] rank %d: TCP data plane (shared device)\n",
              rank);
    }
  }
}

GpuContext::~GpuContext() {
  if (impl_ && impl_->dc.nccl) ncclCommDestroy(impl_->dc.nccl);
}

void GpuContext::device_sync() { HIP_CHECK(hipDeviceSynchronize()); }

std::array<uint64_t, 4> GpuContext::debug_expand_counts(bool reset) {
  std::array<uint64_t, 4> out;
  for (int i = 0; i < kLbCount; ++i) {
    out[i] = impl_->expand_counts[i];
    if (reset) impl_->expand_counts[i] = 0;
  }
  return out;
}

// GRAPEHIP_ARC_DEPTH: the 64-arc windows whose gathers a wave of
// pr_pull_seg_kernel keeps in flight, read once per process. 1, 2 and 4 are
// built; anything else is the default. The small pull and the frontier
// expansion stay at one arc per lane: batched the same way they were slower
// or gained less than the benchmark can show (profiles/r12_arc_depth.md).
constexpr int kArcDepthDefault = 4;

static int arc_depth() {
  static const int depth = [] {
    const char* e = getenv("GRAPEHIP_ARC_DEPTH");
    if (!e || !*e) return kArcDepthDefault;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    return *end == '\0' && (v == 1 || v == 2 || v == 4) ? static_cast<int>(v)
                                                        : kArcDepthDefault;
  }();
  return depth;
}

int GpuContext::debug_arc_depth() { return arc_depth(); }

std::array<uint64_t, 2> GpuContext::debug_pr_path(bool reset) {
  std::array<uint64_t, 2> out = {impl_->pr_path_counts[0],
                                 impl_->pr_path_counts[1]};
  if (reset) impl_->pr_path_counts[0] = impl_->pr_path_counts[1] = 0;
  return out;
}

// GRAPEHIP_PR_EPILOGUE: 0 keeps pagerank() off the epilogue path, read once
// per process.
static bool pr_epilogue_on() {
  static const bool on = [] {
    const char* e = getenv("GRAPEHIP_PR_EPILOGUE");
    return !e || !*e || atoi(e) != 0;
  }();
  return on;
}

std::array<uint64_t, 2> GpuContext::debug_pr_epilogue(bool reset) {
  std::array<uint64_t, 2> out = {impl_->pr_epi_counts[0],
                                 impl_->pr_epi_counts[1]};
  if (reset) impl_->pr_epi_counts[0] = impl_->pr_epi_counts[1] = 0;
  return out;
}

std::vector<uint64_t> GpuContext::debug_scan(const std::vector<uint32_t>& in) {
  hipStream_t s = impl_->compute;
  DeviceBuffer<uint32_t> d_in;
  d_in.upload(in, s);
  DeviceBuffer<uint64_t> d_out(in.size() + 1);
  exclusive_scan(d_in.data(), d_out.data(), in.size(), s, impl_->scan);
  return d_out.download(s);
}

std::vector<uint32_t> GpuContext::debug_sort_rows(
    const std::vector<uint64_t>& off, std::vector<uint32_t> dst,
    std::vector<float>* w) {
  if (off.empty()) return dst;
  if (off.back() > dst.size() || (w && w->size() != dst.size()))
    throw std::runtime_error("debug_sort_rows: offsets do not match the keys");
  if (!std::is_sorted(off.begin(), off.end()) || off.size() > 0xFFFFFFFFull)
    throw std::runtime_error("debug_sort_rows: offsets must ascend");
  hipStream_t s = impl_->compute;
  const uint32_t rows_n = static_cast<uint32_t>(off.size() - 1);
  DeviceBuffer<uint64_t> d_off;
  d_off.upload(off, s);
  DeviceBuffer<uint32_t> d_dst(dst.size() ? dst.size() : 1);
  DeviceBuffer<float> d_w(w && dst.size() ? dst.size() : 1);
  if (!dst.empty()) {
    HIP_CHECK(hipMemcpyAsync(d_dst.data(), dst.data(), dst.size() * 4,
                             hipMemcpyHostToDevice, s));
    if (w)
      HIP_CHECK(hipMemcpyAsync(d_w.data(), w->data(), dst.size() * 4,
                               hipMemcpyHostToDevice, s));
  }
  if (w)
    segmented_sort_rows(d_off.data(), rows_n,
                        PairKeyCodec{d_dst.data(), d_w.data()}, s,
                        impl_->scan);
  else
    segmented_sort_rows(d_off.data(), rows_n, U32KeyCodec{d_dst.data()}, s,
                        impl_->scan);
  if (!dst.empty()) {
    HIP_CHECK(hipMemcpyAsync(dst.data(), d_dst.data(), dst.size() * 4,
                             hipMemcpyDeviceToHost, s));
    if (w)
      HIP_CHECK(hipMemcpyAsync(w->data(), d_w.data(), dst.size() * 4,
                               hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return dst;
}

// ---------------------------------------------------------------------------
// Graph construction
// ---------------------------------------------------------------------------

namespace {

void build_csr_from_coo(const DeviceBuffer<uint32_t>& src,
                        const DeviceBuffer<uint32_t>& dst,
                        const DeviceBuffer<float>& w, uint64_t n,
                        uint32_t v_begin, uint32_t owned, bool weighted,
                        DeviceBuffer<uint64_t>& out_off,
                        DeviceBuffer<uint32_t>& out_dst,
                        DeviceBuffer<float>& out_w, hipStream_t s,
                        ScanTemp& scan) {
  DeviceBuffer<uint32_t> deg(owned);
  deg.zero(s);
  if (n)
    count_deg_kernel<<<grid_for(n), kBlock, 0, s>>>(src.data(), n, v_begin,
                                                    deg.data());
  out_off.resize(owned + 1);
  uint64_t total = exclusive_scan(deg.data(), out_off.data(), owned, s, scan);
  if (getenv("GRAPEHIP_DEBUG"))
    fprintf(stderr, "[csr] scan total=%lu n=%lu\n", (unsigned long)total,
            (unsigned long)n);
  if (total != n) throw std::runtime_error("CSR build: degree sum mismatch");
  deg.free();
  DeviceBuffer<unsigned long long> cursor(owned);
  HIP_CHECK(hipMemcpyAsync(cursor.data(), out_off.data(), owned * 8,
                           hipMemcpyDeviceToDevice, s));
  out_dst.resize(total);
  if (weighted) out_w.resize(total);
  if (n)
    scatter_edges_kernel<<<grid_for(n), kBlock, 0, s>>>(
        src.data(), dst.data(), weighted ? w.data() : nullptr, n, v_begin,
        cursor.data(), out_dst.data(), weighted ? out_w.data() : nullptr);
  HIP_CHECK(hipStreamSynchronize(s));
}

void sort_csr_rows(const DeviceBuffer<uint64_t>& off,
                   DeviceBuffer<uint32_t>& dst, DeviceBuffer<float>* w,
                   uint32_t rows_n, hipStream_t s, ScanTemp& scan) {
  if (rows_n == 0) return;
  segmented_sort_rows(off.data(), rows_n,
                      PairKeyCodec{dst.data(), w ? w->data() : nullptr}, s,
                      scan);
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

std::unique_ptr<DeviceGraph> GpuContext::gen_synthetic(
    uint64_t nv, uint64_t ne, uint64_t seed, bool directed, bool weighted,
    bool build_in_csr, double a, double b, double c) {
  if (nv >= (1ull << 32))
    throw std::runtime_error("gen_synthetic: nv must fit in 32 bits");
  auto g = std::make_unique<DeviceGraph>();
  g->nv_global = static_cast<uint32_t>(nv);
  g->nv_real = nv;
  g->directed = directed;
  g->weighted = weighted;
  g->input_edges = ne;
  uint32_t slice = static_cast<uint32_t>((nv + world_ - 1) / world_);
  g->seg_host.resize(world_ + 1);
  for (int f = 0; f <= world_; ++f)
    g->seg_host[f] = static_cast<uint32_t>(
        std::min<uint64_t>(static_cast<uint64_t>(f) * slice, nv));
  g->seg.upload(g->seg_host, impl_->compute);
  g->v_begin = g->seg_host[rank_];
  g->v_end = g->seg_host[rank_ + 1];
  uint32_t owned = g->owned();
  g->owned_real = owned;

  int scale = 0;
  while ((1ull << scale) < nv) ++scale;
  uint32_t t_a = static_cast<uint32_t>(a * 65536.0);
  uint32_t t_ab = static_cast<uint32_t>((a + b) * 65536.0);
  uint32_t t_abc = static_cast<uint32_t>((a + b + c) * 65536.0);
  // slice-balance scramble (see gen_edges_kernel); deterministic per nv
  uint64_t scr_a = 0, scr_b = 0;
  if (!(getenv("GRAPEHIP_SCRAMBLE") &&
        atoi(getenv("GRAPEHIP_SCRAMBLE")) == 0) && nv > 2) {
    scr_a = static_cast<uint64_t>(nv * 0.6180339887498949);
    if (scr_a < 2) scr_a = 2;
    auto gcd_u64 = [](uint64_t x, uint64_t y) {
      while (y) {
        uint64_t t = x % y;
        x = y;
        y = t;
      }
      return x;
    };
    while (gcd_u64(scr_a, nv) != 1) ++scr_a;
    scr_b = (seed * 0x9E3779B97F4A7C15ULL) % nv;
  }

  hipStream_t s = impl_->compute;
  // exact per-rank edge count via a counting pass (see gen_edges_kernel)
  DeviceBuffer<unsigned long long> cnt(1);
  cnt.zero(s);
  uint64_t est;
  if (world_ == 1) {
    est = static_cast<uint64_t>((directed ? 1.0 : 2.0) * ne) + 16;
  } else {
    gen_edges_kernel<<<kMaxGrid, kBlock, 0, s>>>(
        ne, seed, scale, g->nv_global, t_a, t_ab, t_abc, scr_a, scr_b,
        g->v_begin, g->v_end, !directed, false, false, nullptr, nullptr,
        nullptr, cnt.data());
    unsigned long long c = 0;
    HIP_CHECK(hipMemcpyAsync(&c, cnt.data(), 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    est = c + 16;
    cnt.zero(s);
  }
  DeviceBuffer<uint32_t> e_src(est), e_dst(est);
  DeviceBuffer<float> e_w(weighted ? est : 0);
  if (getenv("GRAPEHIP_DEBUG"))
    fprintf(stderr, "[gen] nv=%u ne=%lu est=%lu scale=%d\n", g->nv_global,
            (unsigned long)ne, (unsigned long)est, scale);
  gen_edges_kernel<<<kMaxGrid, kBlock, 0, s>>>(
      ne, seed, scale, g->nv_global, t_a, t_ab, t_abc, scr_a, scr_b, g->v_begin, g->v_end,
      !directed, false, weighted, e_src.data(), e_dst.data(),
      weighted ? e_w.data() : nullptr, cnt.data());
  unsigned long long n_local = 0;
  HIP_CHECK(hipMemcpyAsync(&n_local, cnt.data(), 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (n_local > est) throw std::runtime_error("gen_synthetic: overflow");
  if (getenv("GRAPEHIP_DEBUG"))
    fprintf(stderr, "[gen] n_local=%llu\n", n_local);

  // hub-clustering renumber: order each slice by descending appearance
  // count (out-stream src count = how often an id is REFERENCED by pull
  // gathers: full degree when undirected, out-degree when directed).
  // Counting sort over capped degrees; within-bucket order is arbitrary.
  const bool renumber =
      !(getenv("GRAPEHIP_RENUMBER") &&
        atoi(getenv("GRAPEHIP_RENUMBER")) == 0);
  if (renumber) {
    uint32_t nv_pad = padded_nv(*g, world_);
    DeviceBuffer<uint32_t> deg(owned ? owned : 1);
    deg.zero(s);
    if (n_local)
      count_deg_kernel<<<grid_for(n_local), kBlock, 0, s>>>(
          e_src.data(), n_local, g->v_begin, deg.data());
    DeviceBuffer<unsigned long long> hist(kRenumBuckets);
    hist.zero(s);
    if (owned)
      renum_hist_kernel<<<grid_for(owned), kBlock, 0, s>>>(
          deg.data(), owned, hist.data());
    auto h = hist.download(s);
    // descending bucket offsets (bucket 4095 = hottest, first)
    std::vector<unsigned long long> cur_h(kRenumBuckets);
    unsigned long long run = 0;
    for (int b = kRenumBuckets - 1; b >= 0; --b) {
      cur_h[b] = run;
      run += h[b];
    }
    DeviceBuffer<unsigned long long> cur;
    cur.upload(cur_h, s);
    g->perm.resize(nv_pad);
    iota_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(g->perm.data(), 0,
                                                    nv_pad);
    if (owned)
      renum_scatter_kernel<<<grid_for(owned), kBlock, 0, s>>>(
          deg.data(), owned, g->v_begin, cur.data(), g->perm.data());
    if (world_ > 1)
      impl_->dc.allgather32(g->perm.data(), slice, false, s);
    if (n_local) {
      remap_ids_kernel<<<grid_for(n_local), kBlock, 0, s>>>(
          e_src.data(), n_local, g->perm.data());
      remap_ids_kernel<<<grid_for(n_local), kBlock, 0, s>>>(
          e_dst.data(), n_local, g->perm.data());
    }
    g->inv.resize(nv_pad);
    inv_scatter_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(
        g->perm.data(), nv_pad, g->inv.data());
    g->permuted = true;
  }

  build_csr_from_coo(e_src, e_dst, e_w, n_local, g->v_begin, owned, weighted,
                     g->oe_off, g->oe_dst, g->oe_w, s, impl_->scan);
  sort_csr_rows(g->oe_off, g->oe_dst, weighted ? &g->oe_w : nullptr, owned,
                s, impl_->scan);
  if (directed && build_in_csr) {
    // regenerate the SAME edge stream, keeping edges whose dst is owned,
    // reversed — builds the in-CSR without materializing the global list
    if (world_ > 1) {
      // in-edge ownership skews differently than out; recount exactly
      cnt.zero(s);
      gen_edges_kernel<<<kMaxGrid, kBlock, 0, s>>>(
          ne, seed, scale, g->nv_global, t_a, t_ab, t_abc, scr_a, scr_b, g->v_begin,
          g->v_end, false, true, false, nullptr, nullptr, nullptr,
          cnt.data());
      unsigned long long c_in = 0;
      HIP_CHECK(hipMemcpyAsync(&c_in, cnt.data(), 8, hipMemcpyDeviceToHost,
                               s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (c_in + 16 > est) {
        est = c_in + 16;
        e_src.free();
        e_dst.free();
        e_w.free();
        e_src.resize(est);
        e_dst.resize(est);
        if (weighted) e_w.resize(est);
      }
    }
    cnt.zero(s);
    gen_edges_kernel<<<kMaxGrid, kBlock, 0, s>>>(
        ne, seed, scale, g->nv_global, t_a, t_ab, t_abc, scr_a, scr_b, g->v_begin,
        g->v_end, false, true, weighted, e_src.data(), e_dst.data(),
        weighted ? e_w.data() : nullptr, cnt.data());
    unsigned long long n_in = 0;
    HIP_CHECK(hipMemcpyAsync(&n_in, cnt.data(), 8, hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (n_in > est) throw std::runtime_error("gen_synthetic: in overflow");
    if (g->permuted && n_in) {
      remap_ids_kernel<<<grid_for(n_in), kBlock, 0, s>>>(
          e_src.data(), n_in, g->perm.data());
      remap_ids_kernel<<<grid_for(n_in), kBlock, 0, s>>>(
          e_dst.data(), n_in, g->perm.data());
    }
    build_csr_from_coo(e_src, e_dst, e_w, n_in, g->v_begin, owned, weighted,
                       g->ie_off, g->ie_dst, g->ie_w, s, impl_->scan);
    sort_csr_rows(g->ie_off, g->ie_dst, weighted ? &g->ie_w : nullptr,
                  owned, s, impl_->scan);
    g->has_in = true;
  }
  e_src.free();
  e_dst.free();
  e_w.free();
  g->local_edges = n_local;
  g->total_edges = comm_ && world_ > 1 ? comm_->allreduce_sum(n_local)
                                       : n_local;
  return g;
}

std::unique_ptr<DeviceGraph> GpuContext::upload(const Fragment& frag) {
  auto g = std::make_unique<DeviceGraph>();
  g->directed = frag.directed();
  g->weighted = frag.has_weights();
  g->has_in = frag.has_in_csr();
  g->input_edges = frag.input_edges();
  g->total_edges = frag.total_edges();
  g->local_edges = frag.local_edges();
  g->nv_real = frag.total_vertices();
  hipStream_t s = impl_->compute;
  const bool identity = frag.vm().idxer() == IdxerKind::kIdentity;

  // device id mapping. identity maps use oids directly (segmented
  // ownership from the vertex map). Arbitrary-oid (hashmap) maps are
  // DENSELY RENUMBERED on upload: device id = fid * slice + lid with one
  // uniform slice = max fragment vnum, so owner lookup stays v/slice and
  // RCCL slices stay uniform (the reference needs a device hashmap,
  // cuda/vertex_map/device_vertex_map.h, for the same capability).
  // Padding rows [ivnum, slice) get empty adjacency.
  std::function<uint32_t(vid_t)> lid2dev;
  uint32_t slice;
  if (identity) {
    const auto& seg64 = frag.vm().segments();
    g->seg_host.assign(seg64.begin(), seg64.end());
    g->nv_global = static_cast<uint32_t>(frag.total_vertices());
    g->v_begin = g->seg_host[frag.fid()];
    g->v_end = g->seg_host[frag.fid() + 1];
    slice = g->seg_host.size() > 1
                ? static_cast<uint32_t>(g->seg_host[1] - g->seg_host[0])
                : g->nv_global;
    lid2dev = [&frag](vid_t lid) {
      return static_cast<uint32_t>(frag.lid2oid(lid));
    };
  } else {
    uint64_t vmax = frag.ivnum();
    if (comm_ && world_ > 1) vmax = comm_->allreduce_max(vmax);
    slice = static_cast<uint32_t>(vmax);
    g->nv_global = static_cast<uint32_t>(
        static_cast<uint64_t>(slice) * world_);
    g->seg_host.resize(world_ + 1);
    for (int f = 0; f <= world_; ++f)
      g->seg_host[f] = static_cast<uint32_t>(
          static_cast<uint64_t>(f) * slice);
    g->v_begin = g->seg_host[frag.fid()];
    g->v_end = g->seg_host[frag.fid() + 1];
    const IdParser& P = frag.parser();
    lid2dev = [&frag, &P, slice](vid_t lid) {
      vid_t gid = frag.lid2gid(lid);
      return static_cast<uint32_t>(
          static_cast<uint64_t>(P.fid(gid)) * slice + P.lid(gid));
    };
  }
  g->owned_real = identity ? g->owned() : frag.ivnum();
  g->seg.upload(g->seg_host, s);

  auto convert = [&](const std::vector<vid_t>& dst_lid) {
    std::vector<uint32_t> out(dst_lid.size());
    parallel_for(0, dst_lid.size(), [&](size_t i) {
      out[i] = lid2dev(dst_lid[i]);
    }, 8192);
    return out;
  };
  auto pad_offsets = [&](const std::vector<eid_t>& off) {
    // extend to the padded owned range with empty rows
    uint32_t rows = g->v_end - g->v_begin;
    std::vector<eid_t> out(off);
    out.resize(rows + 1, off.empty() ? 0 : off.back());
    return out;
  };
  g->oe_off.upload(pad_offsets(frag.oe_offsets()), s);
  g->oe_dst.upload(convert(frag.oe_dsts()), s);
  if (g->weighted) g->oe_w.upload(frag.oe_weights(), s);
  if (g->has_in) {
    g->ie_off.upload(pad_offsets(frag.ie_offsets()), s);
    g->ie_dst.upload(convert(frag.ie_dsts()), s);
    if (g->weighted) g->ie_w.upload(frag.ie_weights(), s);
  }
  uint32_t owned_rows = g->owned();
  sort_csr_rows(g->oe_off, g->oe_dst, g->weighted ? &g->oe_w : nullptr,
                owned_rows, s, impl_->scan);
  if (g->has_in)
    sort_csr_rows(g->ie_off, g->ie_dst, g->weighted ? &g->ie_w : nullptr,
                  owned_rows, s, impl_->scan);
  if (!identity) {
    // CDLP tie-breaks compare label VALUES; the reference's labels are
    // oids, so under dense renumbering the comparison space must be the
    // global sorted-OID order (vertex map is replicated — every rank
    // derives the identical table)
    const VertexMap& vm = frag.vm();
    const IdParser& P = frag.parser();
    std::vector<std::pair<oid_t, uint32_t>> pairs;
    pairs.reserve(vm.total_vertices());
    for (int f = 0; f < vm.fnum(); ++f) {
      vid_t n = vm.frag_vnum(static_cast<fid_t>(f));
      for (vid_t l = 0; l < n; ++l)
        pairs.emplace_back(
            vm.get_oid(P.gid(static_cast<fid_t>(f), l)),
            static_cast<uint32_t>(static_cast<uint64_t>(f) * slice + l));
    }
    std::sort(pairs.begin(), pairs.end());
    std::vector<uint32_t> order(padded_nv(*g, world_), 0xFFFFFFFFu);
    for (uint32_t i = 0; i < pairs.size(); ++i)
      order[pairs[i].second] = i;
    g->oid_order.upload(order, s);
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return g;
}

}  // namespace grapehip

namespace grapehip {

// ---------------------------------------------------------------------------
// Materialize a bitmap frontier into a queue; returns the count.
// bm covers bits [0, nbits) (owned rows); q entries are global vids
// (bit_base = v_begin). Clears the bitmap.
// ---------------------------------------------------------------------------
static uint64_t compact_frontier(GpuContext::Impl& I, uint32_t* bm_words,
                                 size_t nbits, uint32_t bit_base, uint32_t* q,
                                 hipStream_t s) {
  size_t nwords = (nbits + 31) / 32;
  if (I.frontier_deg.size() < nwords)
    I.frontier_deg.resize(nwords + (nwords >> 2) + 64);
  if (I.frontier_off.size() < nwords + 1)
    I.frontier_off.resize(nwords + (nwords >> 2) + 65);
  popc_words_kernel<<<grid_for(nwords), kBlock, 0, s>>>(bm_words, nwords,
                                                        I.frontier_deg.data());
  uint64_t total = exclusive_scan(I.frontier_deg.data(),
                                  I.frontier_off.data(), nwords, s, I.scan);
  if (total)
    fill_frontier_kernel<<<grid_for(nwords), kBlock, 0, s>>>(
        bm_words, nwords, I.frontier_off.data(), bit_base, q);
  return total;
}

// compact_frontier for a frontier app: returns this rank's count and writes
// the count over all ranks, which every rank needs to leave the loop in the
// same round. One rank: no collective.
static uint32_t compact_frontier_global(GpuContext::Impl& I, TcpComm* comm,
                                        int world, uint32_t* bm_words,
                                        size_t nbits, uint32_t bit_base,
                                        uint32_t* q, hipStream_t s,
                                        uint64_t& global) {
  uint32_t qn = static_cast<uint32_t>(
      compact_frontier(I, bm_words, nbits, bit_base, q, s));
  global = world > 1 ? comm->allreduce_sum(qn) : qn;
  return qn;
}

// ---------------------------------------------------------------------------
// Degree buckets over the pull CSR (undirected: out == neighborhood;
// directed: in-CSR). Built once per graph, reused by PR pull + BFS pull.
// ---------------------------------------------------------------------------

// Also builds rows_active and the hub work list (see DeviceGraph). All of
// it hangs off the DeviceGraph and is built once: a mutated graph is
// re-uploaded as a fresh DeviceGraph, and the cached PageRank hipGraph that
// bakes these pointers is destroyed before the buffers in ~DeviceGraph.
static void ensure_buckets(DeviceGraph& g, GpuContext::Impl& I,
                           hipStream_t s) {
  if (g.buckets_built) return;
  uint32_t owned = g.owned();
  const uint64_t* pull_off = !g.directed ? g.oe_off.data() : g.ie_off.data();
  const uint64_t* out_off = g.oe_off.data();
  auto h = partition_rows(PullDegTiers{pull_off, out_off, g.owned_real},
                          owned, {&g.rows_small, &g.rows_mid, &g.rows_large},
                          s);
  g.n_small = h[0];
  g.n_mid = h[1];
  g.n_large = h[2];
  g.n_isolated_real = h[3];
  g.n_isolated_pad = h[4];

  // rows_active: bitmap of rows with an edge, compacted in ascending order
  g.n_active = owned - g.n_isolated_real - g.n_isolated_pad;
  g.rows_active.resize(g.n_active ? g.n_active : 1);
  // the bitmap stays on the graph (pr_fill_isolated_kernel tests it)
  size_t nwords = (static_cast<size_t>(owned) + 31) / 32;
  g.active_bm.resize(nwords ? nwords : 1);
  active_rows_bitmap_kernel<<<grid_for(nwords), kBlock, 0, s>>>(
      pull_off, out_off, owned, g.active_bm.data(), nwords);
  if (g.n_active) {
    // compact_frontier clears the bitmap it reads: give it a copy
    DeviceBuffer<uint32_t> bm(nwords);
    HIP_CHECK(hipMemcpyAsync(bm.data(), g.active_bm.data(), nwords * 4,
                             hipMemcpyDeviceToDevice, s));
    uint64_t got =
        compact_frontier(I, bm.data(), owned, 0, g.rows_active.data(), s);
    HIP_CHECK(hipStreamSynchronize(s));  // bm is freed on return
    if (got != g.n_active)
      throw std::runtime_error("buckets: active-row count mismatch");
  }

  // hub work list, built on the host: n_large <= E / kMidDeg rows
  g.n_hub_items = 0;
  if (g.n_large) {
    std::vector<uint32_t> rows(g.n_large);
    HIP_CHECK(hipMemcpyAsync(rows.data(), g.rows_large.data(),
                             g.n_large * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    // the block-aggregated reservation leaves the list in no fixed order;
    // sort it so the item order (and with it every hub sum) is the same
    // for every build of the same graph
    std::sort(rows.begin(), rows.end());
    HIP_CHECK(hipMemcpyAsync(g.rows_large.data(), rows.data(),
                             g.n_large * 4, hipMemcpyHostToDevice, s));
    DeviceBuffer<uint64_t> d_deg(g.n_large);
    gather_row_deg_kernel<<<grid_for(g.n_large), kBlock, 0, s>>>(
        pull_off, g.rows_large.data(), g.n_large, d_deg.data());
    auto deg = d_deg.download(s);
    std::vector<uint32_t> item_row, item_seg, row_first(g.n_large + 1);
    for (uint64_t j = 0; j < g.n_large; ++j) {
      row_first[j] = static_cast<uint32_t>(item_row.size());
      uint64_t nseg = (deg[j] + kHubSeg - 1) / kHubSeg;
      if (item_row.size() + nseg > 0xFFFFFFFFull)
        throw std::runtime_error("buckets: hub work list too large");
      for (uint64_t k = 0; k < nseg; ++k) {
        item_row.push_back(static_cast<uint32_t>(j));
        item_seg.push_back(static_cast<uint32_t>(k));
      }
    }
    row_first[g.n_large] = static_cast<uint32_t>(item_row.size());
    g.n_hub_items = item_row.size();
    g.hub_item_row.upload(item_row, s);
    g.hub_item_seg.upload(item_seg, s);
    g.hub_row_first.upload(row_first, s);
    g.pr_hub_part.resize(g.n_hub_items);
    HIP_CHECK(hipStreamSynchronize(s));  // host vectors go out of scope
  }
  if (getenv("GRAPEHIP_DEBUG"))
    fprintf(stderr,
            "[buckets] owned=%u small=%lu mid=%lu large=%lu active=%lu "
            "isolated=%lu isolated_pad=%lu hub_items=%lu\n",
            owned, (unsigned long)g.n_small, (unsigned long)g.n_mid,
            (unsigned long)g.n_large, (unsigned long)g.n_active,
            (unsigned long)g.n_isolated_real,
            (unsigned long)g.n_isolated_pad, (unsigned long)g.n_hub_items);
  g.buckets_built = true;
}

// Knobs of the id-segment pull, read once per process. GRAPEHIP_PR_SEG=0
// selects the row-tier pulls; GRAPEHIP_PR_SEG_HEAD / GRAPEHIP_PR_SEG_IDS set
// the ids of the replicated head and of each slice (tests shrink them to
// reach every segment on tiny graphs); GRAPEHIP_PR_SEG_ITEM the arcs per
// item; GRAPEHIP_PR_SEG_NT=1 streams dst with nontemporal loads.
struct PrSegKnobs {
  bool on;
  uint64_t head, ids;
  uint32_t item;
  bool nt;
};

static const PrSegKnobs& pr_seg_knobs() {
  static const PrSegKnobs k = [] {
    auto num = [](const char* name, uint64_t dflt) {
      const char* e = getenv(name);
      return e && *e ? static_cast<uint64_t>(strtoull(e, nullptr, 10)) : dflt;
    };
    PrSegKnobs r;
    r.on = num("GRAPEHIP_PR_SEG", 1) != 0;
    r.head = num("GRAPEHIP_PR_SEG_HEAD", 256u << 10);
    r.ids = std::max<uint64_t>(num("GRAPEHIP_PR_SEG_IDS", 640u << 10), 1);
    r.item = static_cast<uint32_t>(
        std::max<uint64_t>(num("GRAPEHIP_PR_SEG_ITEM", kHubSeg), kBlock));
    r.nt = num("GRAPEHIP_PR_SEG_NT", 0) != 0;
    return r;
  }();
  return k;
}

// Id-segment layout of the mid and hub rows over the pull CSR, once per
// graph (needs the buckets). Everything is placed by scans over row order,
// so the layout is the same on every build of the same graph. Returns
// whether the path is on for g: it is off when asked off, without a mid or
// hub row, when the segments do not fit below `owned`, or when memory is
// short.
static bool ensure_pr_segments(DeviceGraph& g, GpuContext::Impl& I,
                               hipStream_t s) {
  if (g.pr_seg_state) return g.pr_seg_state > 0;
  g.pr_seg_state = -1;
  const PrSegKnobs& K = pr_seg_knobs();
  const uint32_t owned = g.owned();
  const uint64_t nrows = g.n_mid + g.n_large;
  const uint64_t top = K.head + kPrSlices * K.ids;
  if (!K.on || !nrows || top >= owned) return false;
  const uint64_t n = nrows * kPrSegs;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  // 36 B of scratch and up to 32 B kept per (row, segment), 8 B per item
  if (free_b < n * 68 + (g.local_edges / K.item) * 8 + (512u << 20))
    return false;
  const double t0 = wall_s();
  const uint64_t* pull_off = !g.directed ? g.oe_off.data() : g.ie_off.data();
  const uint32_t* pull_dst = !g.directed ? g.oe_dst.data() : g.ie_dst.data();

  // the rows, ascending (the tier lists are in no fixed order)
  g.seg_rows.resize(nrows);
  {
    size_t nwords = (static_cast<size_t>(owned) + 31) / 32;
    DeviceBuffer<uint32_t> bm(nwords);
    pr_seg_rows_bitmap_kernel<<<grid_for(nwords), kBlock, 0, s>>>(
        pull_off, owned, bm.data(), nwords);
    uint64_t got =
        compact_frontier(I, bm.data(), owned, 0, g.seg_rows.data(), s);
    HIP_CHECK(hipStreamSynchronize(s));  // bm is freed here
    if (got != nrows)
      throw std::runtime_error("pr segments: row count mismatch");
  }

  PrSegBounds bnd;
  for (int k = 0; k <= kPrSegs; ++k) {
    uint64_t b = k == 0 ? 0
                 : k == kPrSegs ? g.nv_global
                                : K.head + (k - 1) * K.ids;
    bnd.b[k] = g.seg_bound[k] = static_cast<uint32_t>(b);
  }

  DeviceBuffer<uint32_t> len(n), flag(n), pieces(n);
  DeviceBuffer<uint64_t> pref(n + 1), sid(n + 1), pfirst(n + 1);
  DeviceBuffer<int> too_long(1);
  too_long.zero(s);
  pr_seg_cut_kernel<<<grid_for(nrows * kWave), kBlock, 0, s>>>(
      pull_off, pull_dst, g.seg_rows.data(), nrows, bnd, len.data(),
      too_long.data());
  g.seg_row_deg.resize(nrows);
  pr_seg_row_deg_kernel<<<grid_for(nrows), kBlock, 0, s>>>(
      pull_off, g.seg_rows.data(), nrows, g.seg_row_deg.data(),
      too_long.data());
  if (too_long.download(s)[0]) return false;
  exclusive_scan(len.data(), pref.data(), n, s, I.scan);
  pr_seg_pieces_kernel<<<grid_for(n), kBlock, 0, s>>>(
      len.data(), pref.data(), nrows, K.item, flag.data(), pieces.data());
  g.n_seg_spans = exclusive_scan(flag.data(), sid.data(), n, s, I.scan);
  g.n_seg_parts = exclusive_scan(pieces.data(), pfirst.data(), n, s, I.scan);
  if (g.n_seg_parts > 0xFFFFFFFFull) return false;

  g.seg_span_pref.resize(g.n_seg_spans + 1);
  g.seg_span_base.resize(g.n_seg_spans);
  g.seg_span_row.resize(g.n_seg_spans);
  g.seg_span_slot.resize(g.n_seg_spans);
  g.seg_row_first.resize(nrows + 1);
  g.seg_part.resize(g.n_seg_parts);
  g.seg_ctr.resize(kPrSegs);
  pr_seg_fill_kernel<<<grid_for(n), kBlock, 0, s>>>(
      len.data(), pref.data(), sid.data(), pfirst.data(), pull_off,
      g.seg_rows.data(), nrows, g.seg_span_pref.data(),
      g.seg_span_base.data(), g.seg_span_row.data(), g.seg_span_slot.data(),
      g.seg_row_first.data());

  PrSegView& v = g.seg_view;
  for (int k = 0; k <= kPrSegs; ++k) {
    HIP_CHECK(hipMemcpyAsync(&v.span_first[k], sid.data() + k * nrows, 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&v.arc_first[k], pref.data() + k * nrows, 8,
                             hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));  // the scratch goes out of scope
  for (int k = 0; k < kPrSegs; ++k) {
    uint64_t items =
        (v.arc_first[k + 1] - v.arc_first[k] + K.item - 1) / K.item;
    if (items > 0x7FFFFFFFull) return false;
    v.n_items[k] = static_cast<uint32_t>(items);
  }
  v.item = K.item;
  v.span_pref = g.seg_span_pref.data();
  v.span_base = g.seg_span_base.data();
  v.span_slot = g.seg_span_slot.data();
  g.n_seg_rows = nrows;
  g.pr_seg_build_ms = (wall_s() - t0) * 1e3;
  if (getenv("GRAPEHIP_DEBUG")) {
    fprintf(stderr,
            "[pr segments] rows=%lu spans=%lu partials=%lu head=%lu ids=%lu "
            "item=%u build=%.1fms kept=%.1fMB items:",
            (unsigned long)nrows, (unsigned long)g.n_seg_spans,
            (unsigned long)g.n_seg_parts, (unsigned long)K.head,
            (unsigned long)K.ids, K.item, g.pr_seg_build_ms,
            (g.n_seg_spans * 24.0 + g.n_seg_parts * 8.0 + nrows * 16.0) / 1e6);
    for (int k = 0; k < kPrSegs; ++k) fprintf(stderr, " %u", v.n_items[k]);
    fprintf(stderr, "\n");
  }
  g.pr_seg_state = 1;
  return true;
}

GpuContext::PrSegDebug GpuContext::debug_pr_segments(DeviceGraph& g) {
  auto& I = *impl_;
  hipStream_t s = I.compute;
  PrSegDebug d;
  if (world_ > 1 || (g.directed && !g.has_in)) return d;
  ensure_buckets(g, I, s);
  d.on = ensure_pr_segments(g, I, s);
  d.off = (!g.directed ? g.oe_off : g.ie_off).download(s);
  d.dst = (!g.directed ? g.oe_dst : g.ie_dst).download(s);
  if (!d.on) return d;
  d.item = g.seg_view.item;
  d.bound.assign(g.seg_bound, g.seg_bound + kPrSegs + 1);
  d.span_first.assign(g.seg_view.span_first,
                      g.seg_view.span_first + kPrSegs + 1);
  d.rows = g.seg_rows.download(s);
  d.span_row = g.seg_span_row.download(s);
  d.span_slot = g.seg_span_slot.download(s);
  d.span_pref = g.seg_span_pref.download(s);
  d.span_base = g.seg_span_base.download(s);
  d.row_first = g.seg_row_first.download(s);
  d.build_ms = g.pr_seg_build_ms;
  d.bytes = g.n_seg_spans * 24 + 8 + g.n_seg_parts * 8 +
            g.n_seg_rows * 16 + 8;
  return d;
}

GpuContext::CsrDebug GpuContext::debug_csr(const DeviceGraph& g) {
  if (world_ > 1)
    throw std::runtime_error("debug_csr: single-GPU graphs only");
  hipStream_t s = impl_->compute;
  // an empty buffer has no device pointer to copy from
  auto get = [s](const auto& b) {
    return b.size() ? b.download(s) : decltype(b.download(s)){};
  };
  CsrDebug d;
  d.v_begin = g.v_begin;
  d.weighted = g.weighted;
  d.has_in = g.has_in;
  d.permuted = g.permuted;
  d.off = get(g.oe_off);
  d.dst = get(g.oe_dst);
  if (g.weighted) d.w = get(g.oe_w);
  if (g.has_in) {
    d.in_off = get(g.ie_off);
    d.in_dst = get(g.ie_dst);
    if (g.weighted) d.in_w = get(g.ie_w);
  }
  if (g.permuted) {
    d.old_of_new = get(g.inv);
    d.new_of_old = get(g.perm);
  }
  return d;
}

static void ensure_pr_tiles(DeviceGraph& g, GpuContext::Impl& I,
                            hipStream_t s) {
  if (g.pr_tiles_built) return;
  const uint64_t* pull_off = !g.directed ? g.oe_off.data() : g.ie_off.data();
  const uint32_t* pull_dst = !g.directed ? g.oe_dst.data() : g.ie_dst.data();
  uint64_t ne = !g.directed ? g.oe_dst.size() : g.ie_dst.size();
  uint32_t ntiles =
      (g.nv_global + (1u << kPrTileBits) - 1) >> kPrTileBits;
  // memory gate: 8 B/edge for the stream + counters; fall back to the
  // row-major pull when HBM is tight (huge 1B+-vertex graphs)
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (free_b < ne * 8 + (static_cast<size_t>(ntiles) + 2) * 16 + (512u << 20)) {
    g.pr_tiles_built = true;  // decided: stay on fallback
    g.pr_ntiles = 0;
    return;
  }
  DeviceBuffer<unsigned long long> cnt(ntiles + 1);
  cnt.zero(s);
  auto runs = [&](unsigned long long* c, unsigned long long* out) {
    if (g.n_small)
      pr_tile_runs_small_kernel<<<grid_for(g.n_small), kBlock, 0, s>>>(
          pull_off, pull_dst, g.rows_small.data(), g.n_small, g.v_begin, c,
          out);
    if (g.n_mid)
      pr_tile_runs_wave_kernel<<<grid_for(g.n_mid * kWave), kBlock, 0, s>>>(
          pull_off, pull_dst, g.rows_mid.data(), g.n_mid, g.v_begin, c, out);
    if (g.n_large)
      pr_tile_runs_wave_kernel<<<std::min<uint64_t>(g.n_large, kMaxGrid),
                                 kBlock, 0, s>>>(
          pull_off, pull_dst, g.rows_large.data(), g.n_large, g.v_begin, c,
          out);
  };
  runs(cnt.data(), nullptr);
  g.pr_tile_off.resize(static_cast<size_t>(ntiles) + 1);
  exclusive_scan(cnt.data(), g.pr_tile_off.data(), ntiles, s, I.scan);
  g.pr_tiles.resize(ne ? ne : 1);
  // cursors = copy of offsets
  DeviceBuffer<unsigned long long> cur(ntiles + 1);
  HIP_CHECK(hipMemcpyAsync(cur.data(), g.pr_tile_off.data(),
                           (static_cast<size_t>(ntiles) + 1) * 8,
                           hipMemcpyDeviceToDevice, s));
  runs(cur.data(), g.pr_tiles.data());
  // host copies of the slice-boundary tile offsets for the phase split
  uint32_t t0 = (g.v_begin + (1u << kPrTileBits) - 1) >> kPrTileBits;
  uint32_t t1 = g.v_end >> kPrTileBits;
  if (t1 < t0) t1 = t0;
  if (t1 > ntiles) t1 = ntiles;
  uint64_t v[3] = {0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(&v[0], g.pr_tile_off.data() + t0, 8,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&v[1], g.pr_tile_off.data() + t1, 8,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&v[2], g.pr_tile_off.data() + ntiles, 8,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  g.pr_own_lo = v[0];
  g.pr_own_hi = v[1];
  g.pr_total = v[2];
  g.pr_ntiles = ntiles;
  g.pr_tiles_built = true;
}

// ---------------------------------------------------------------------------
// Halo host-side flush: pack per-peer pairs, exchange counts over TCP,
// ncclSend/Recv payloads over xGMI. Returns #received pairs (in recvbuf).
// TAKE packs with halo_pack_take_kernel: the packed state entries are zero
// again afterwards (accumulators such as the k-core decrement counts).
// ---------------------------------------------------------------------------
template <typename T, bool TAKE = false>
uint64_t halo_flush(GpuContext::Impl& I, TcpComm* comm, int rank, int world,
                    std::conditional_t<TAKE, T*, const T*> state,
                    uint64_t cap, hipStream_t s) {
  std::vector<unsigned long long> cnts(world);
  HIP_CHECK(hipMemcpyAsync(cnts.data(), I.halo_cnt.data(), world * 8,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));  // the one inherent host sync: the
                                       // pack launch shapes need the counts
  uint64_t send_total = 0;
  for (int p = 0; p < world; ++p) send_total += cnts[p];
  size_t pair_sz = sizeof(HaloPair<T>);
  if (I.sendbuf.size() < send_total * pair_sz)
    I.sendbuf.resize(send_total * pair_sz + (1 << 20));
  // pack contiguously in peer order (async: runs while the TCP count
  // matrix goes around on the host below)
  std::vector<uint64_t> send_off(world + 1, 0);
  for (int p = 0; p < world; ++p)
    send_off[p + 1] = send_off[p] + cnts[p] * pair_sz;
  for (int p = 0; p < world; ++p) {
    if (!cnts[p]) continue;
    const uint32_t* idx = I.halo_idx.data() + static_cast<uint64_t>(p) * cap;
    auto* out = reinterpret_cast<HaloPair<T>*>(I.sendbuf.data() + send_off[p]);
    if constexpr (TAKE)
      halo_pack_take_kernel<T><<<grid_for(cnts[p]), kBlock, 0, s>>>(
          idx, cnts[p], state, DevBitmap{I.halo_bm.data()}, out);
    else
      halo_pack_kernel<T><<<grid_for(cnts[p]), kBlock, 0, s>>>(
          idx, cnts[p], state, DevBitmap{I.halo_bm.data()}, out);
  }
  I.halo_cnt.zero(s);
  // exchange the count matrix on the control plane
  std::vector<uint64_t> matrix(static_cast<size_t>(world) * world);
  std::vector<uint64_t> mine(cnts.begin(), cnts.end());
  comm->allgather(mine.data(), world * 8, matrix.data());
  uint64_t recv_total = 0;
  std::vector<uint64_t> recv_off(world + 1, 0);
  for (int p = 0; p < world; ++p) {
    uint64_t from_p = matrix[static_cast<size_t>(p) * world + rank];
    recv_off[p + 1] = recv_off[p] + from_p * pair_sz;
    recv_total += from_p;
  }
  if (I.recvbuf.size() < recv_total * pair_sz)
    I.recvbuf.resize(recv_total * pair_sz + (1 << 20));
  // payloads over xGMI on the comm stream, event-ordered after the packs
  // (reference gpu_message_manager.h:401-445 dual-stream design); no host
  // sync — the caller's halo_process launch on `s` waits on ev_comm.
  I.ev_pack.record(s);
  I.ev_pack.wait_on(I.comm_stream);
  I.dc.sendrecv(I.sendbuf.data(), send_off, I.recvbuf.data(), recv_off,
                I.comm_stream);
  I.ev_comm.record(I.comm_stream);
  I.ev_comm.wait_on(s);
  // self pairs (should be none — owned handled locally)
  return recv_total;
}

// Sizes the halo scratch for `cap` indices per peer and a dedup bitmap of
// bm_words, and returns the device handle the push functors carry. A single
// rank sizes nothing: its handle holds whatever the buffers hold and is
// never dereferenced.
static DevHalo halo_reserve(GpuContext::Impl& I, int world, uint64_t cap,
                            uint32_t slice, uint64_t bm_words) {
  if (world > 1) {
    I.halo_idx.resize(static_cast<uint64_t>(world) * cap);
    I.halo_cnt.resize(world);
    I.halo_bm.resize(bm_words);
  }
  return DevHalo{I.halo_idx.data(), I.halo_cnt.data(),
                 DevBitmap{I.halo_bm.data()}, cap, slice, world};
}

// Empties the halo scratch (multi-rank callers only).
static void halo_reset(GpuContext::Impl& I, hipStream_t s) {
  I.halo_cnt.zero(s);
  I.halo_bm.zero(s);
}

// One halo round: flush this rank's pairs to their owners, then apply the
// received pairs with recv_op (multi-rank callers only).
template <typename T, bool TAKE = false, typename RecvOp>
void halo_round(GpuContext::Impl& I, TcpComm* comm, int rank, int world,
                std::conditional_t<TAKE, T*, const T*> state, uint64_t cap,
                RecvOp recv_op, hipStream_t s) {
  uint64_t nrecv = halo_flush<T, TAKE>(I, comm, rank, world, state, cap, s);
  if (nrecv)
    halo_process_kernel<T, RecvOp><<<grid_for(nrecv), kBlock, 0, s>>>(
        reinterpret_cast<HaloPair<T>*>(I.recvbuf.data()), nrecv, recv_op);
}

// ===========================================================================
// Mirror topology: per-peer lists of the remote vertices this rank's edges
// reference (reference mirror-info + BatchShuffle, edgecut_fragment_base.h
// :569+ / cuda batch_shuffle_message_manager.h:81-103). Built once per
// graph; per-round dense refreshes then ship ONLY referenced values,
// point-to-point — each peer pair on its own xGMI link — instead of
// allgathering whole slices around the ring (O(V·world) volume and
// per-link serialization). 4-byte element specialization (depth u32,
// PR contrib f32, CDLP label u32).
// ===========================================================================

__global__ void mark_dsts_kernel(const uint32_t* __restrict__ dst,
                                 uint64_t n, uint32_t v_begin,
                                 uint32_t v_end, DevBitmap bm) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride) {
    uint32_t v = dst[i];
    if (v < v_begin || v >= v_end) (void)bm.set_once(v);
  }
}

// out[t] = lower_bound(idx[0..n), t*slice) for t in [0, world]
__global__ void slice_bounds_kernel(const uint32_t* __restrict__ idx,
                                    uint64_t n, uint32_t slice, int world,
                                    uint64_t* __restrict__ out) {
  int t = threadIdx.x;
  if (t > world) return;
  uint64_t key = static_cast<uint64_t>(t) * slice;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    uint64_t m = (lo + hi) >> 1;
    if (idx[m] < key) lo = m + 1;
    else hi = m;
  }
  out[t] = lo;
}

__global__ void gather4_kernel(const uint32_t* __restrict__ idx, uint64_t n,
                               const uint32_t* __restrict__ state,
                               uint32_t* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride)
    out[i] = state[idx[i]];
}

__global__ void scatter4_kernel(const uint32_t* __restrict__ idx, uint64_t n,
                                const uint32_t* __restrict__ in,
                                uint32_t* __restrict__ state) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride)
    state[idx[i]] = in[i];
}

// Build per-peer request lists from a referenced bitmap (consumed/cleared).
// recv_idx: ascending global ids this rank wants values for, regioned per
// owner; send_idx: the ids each peer wants from this rank's slice.
// Returns the recv total.
static uint64_t build_ref_lists(GpuContext::Impl& I, TcpComm* comm,
                                DeviceBuffer<uint32_t>& bm, size_t nwords,
                                uint32_t slice, int rank, int world,
                                DeviceBuffer<uint32_t>& recv_idx,
                                std::vector<uint64_t>& recv_off,
                                DeviceBuffer<uint32_t>& send_idx,
                                std::vector<uint64_t>& send_off,
                                hipStream_t s) {
  // compact ascending (popc + scan + fill, cleared as it fills)
  if (I.frontier_deg.size() < nwords)
    I.frontier_deg.resize(nwords + (nwords >> 2) + 64);
  if (I.frontier_off.size() < nwords + 1)
    I.frontier_off.resize(nwords + (nwords >> 2) + 65);
  popc_words_kernel<<<grid_for(nwords), kBlock, 0, s>>>(bm.data(), nwords,
                                                        I.frontier_deg.data());
  uint64_t total = exclusive_scan(I.frontier_deg.data(),
                                  I.frontier_off.data(), nwords, s, I.scan);
  recv_idx.resize(total ? total : 1);
  if (total)
    fill_frontier_kernel<<<grid_for(nwords), kBlock, 0, s>>>(
        bm.data(), nwords, I.frontier_off.data(), 0, recv_idx.data());
  // per-peer boundaries (vid-ascending list, slice-contiguous regions)
  DeviceBuffer<uint64_t> d_bounds(world + 1);
  slice_bounds_kernel<<<1, world + 1, 0, s>>>(recv_idx.data(), total, slice,
                                              world, d_bounds.data());
  recv_off = d_bounds.download(s);
  // counts matrix on the control plane -> send-side region sizes
  std::vector<uint64_t> mine(world);
  for (int p = 0; p < world; ++p) mine[p] = recv_off[p + 1] - recv_off[p];
  std::vector<uint64_t> matrix(static_cast<size_t>(world) * world);
  comm->allgather(mine.data(), world * 8, matrix.data());
  send_off.assign(world + 1, 0);
  for (int q = 0; q < world; ++q)
    send_off[q + 1] =
        send_off[q] +
        (q == rank ? 0 : matrix[static_cast<size_t>(q) * world + rank]);
  uint64_t total_send = send_off[world];
  send_idx.resize(total_send ? total_send : 1);
  // ship each peer its request list; receive who wants what from us
  std::vector<uint64_t> sb(world + 1), rb(world + 1);
  for (int p = 0; p <= world; ++p) {
    sb[p] = recv_off[p] * 4;    // my requests, region p -> peer p
    rb[p] = send_off[p] * 4;    // peer q's requests for my slice
  }
  I.dc.sendrecv(reinterpret_cast<const uint8_t*>(recv_idx.data()), sb,
                reinterpret_cast<uint8_t*>(send_idx.data()), rb, s);
  HIP_CHECK(hipStreamSynchronize(s));
  return total;
}

static void ensure_mirrors(GpuContext::Impl& I, TcpComm* comm,
                           DeviceGraph& g, int rank, int world,
                           hipStream_t s) {
  if (g.mirrors_built || world <= 1) return;
  uint32_t nv_pad = padded_nv(g, world);
  uint32_t slice = g.seg_host.size() > 1 ? g.seg_host[1] - g.seg_host[0]
                                         : g.nv_global;
  size_t nwords = (static_cast<size_t>(nv_pad) + 31) / 32;
  DeviceBuffer<uint32_t> bm(nwords);
  bm.zero(s);
  if (g.local_edges)
    mark_dsts_kernel<<<grid_for(g.local_edges), kBlock, 0, s>>>(
        g.oe_dst.data(), g.local_edges, g.v_begin, g.v_end, DevBitmap{bm.data()});
  if (g.has_in && g.ie_dst.size())
    mark_dsts_kernel<<<grid_for(g.ie_dst.size()), kBlock, 0, s>>>(
        g.ie_dst.data(), g.ie_dst.size(), g.v_begin, g.v_end,
        DevBitmap{bm.data()});
  uint64_t total =
      build_ref_lists(I, comm, bm, nwords, slice, rank, world,
                      g.mr_recv_idx, g.mr_recv_off, g.mr_send_idx,
                      g.mr_send_off, s);
  uint64_t total_send = g.mr_send_off[world];
  g.mr_sendbuf.resize(total_send * 4 + 4);
  g.mr_recvbuf.resize(total * 4 + 4);
  g.mirrors_built = true;
  if (getenv("GRAPEHIP_DEBUG"))
    fprintf(stderr,
            "[mirror] rank %d: recv %lu refs, send %lu (slice %u)\n", rank,
            (unsigned long)total, (unsigned long)total_send, slice);
}

// Refresh referenced remote entries of a 4-byte-element state array over
// arbitrary request lists. begin() packs on the compute stream and
// launches the exchange on the comm stream; independent local work may
// run between begin and end — end() orders the scatter after payloads
// land.
static void ref_sync_begin(GpuContext::Impl& I,
                           const DeviceBuffer<uint32_t>& send_idx,
                           const std::vector<uint64_t>& send_off,
                           const std::vector<uint64_t>& recv_off,
                           DeviceBuffer<uint8_t>& sendbuf,
                           DeviceBuffer<uint8_t>& recvbuf,
                           const void* state4, hipStream_t s) {
  uint64_t ns = send_off.back();
  if (ns)
    gather4_kernel<<<grid_for(ns), kBlock, 0, s>>>(
        send_idx.data(), ns, static_cast<const uint32_t*>(state4),
        reinterpret_cast<uint32_t*>(sendbuf.data()));
  I.ev_pack.record(s);
  I.ev_pack.wait_on(I.comm_stream);
  std::vector<uint64_t> sb(send_off.size()), rb(recv_off.size());
  for (size_t p = 0; p < sb.size(); ++p) sb[p] = send_off[p] * 4;
  for (size_t p = 0; p < rb.size(); ++p) rb[p] = recv_off[p] * 4;
  I.dc.sendrecv(sendbuf.data(), sb, recvbuf.data(), rb, I.comm_stream);
  I.ev_comm.record(I.comm_stream);
}

static void ref_sync_end(GpuContext::Impl& I,
                         const DeviceBuffer<uint32_t>& recv_idx,
                         const std::vector<uint64_t>& recv_off,
                         const DeviceBuffer<uint8_t>& recvbuf, void* state4,
                         hipStream_t s) {
  I.ev_comm.wait_on(s);
  uint64_t nr = recv_off.back();
  if (nr)
    scatter4_kernel<<<grid_for(nr), kBlock, 0, s>>>(
        recv_idx.data(), nr,
        reinterpret_cast<const uint32_t*>(recvbuf.data()),
        static_cast<uint32_t*>(state4));
}

static void mirror_sync_begin(GpuContext::Impl& I, DeviceGraph& g,
                              const void* state4, hipStream_t s) {
  ref_sync_begin(I, g.mr_send_idx, g.mr_send_off, g.mr_recv_off,
                 g.mr_sendbuf, g.mr_recvbuf, state4, s);
}

static void mirror_sync_end(GpuContext::Impl& I, DeviceGraph& g,
                            void* state4, hipStream_t s) {
  ref_sync_end(I, g.mr_recv_idx, g.mr_recv_off, g.mr_recvbuf, state4, s);
}

// Changed-gated sparse refresh: ship only (id, value) pairs whose OWNED
// row is marked in `chg` (bit index = id - v_begin). Converging apps
// (CDLP late iterations) change few labels — the dense mirror refresh
// would re-ship every referenced value regardless. Pair order within a
// peer is irrelevant (receiver scatters by id), so packing appends with
// plain atomic cursors into capacity regions; per-round counts ride the
// control plane.
__global__ void mirror_pack_sparse_kernel(
    const uint32_t* __restrict__ send_idx, uint64_t b, uint64_t e,
    const uint32_t* __restrict__ chg_words, uint32_t v_begin,
    const uint32_t* __restrict__ state, unsigned long long* __restrict__ cnt,
    unsigned long long* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = b + blockIdx.x * blockDim.x + threadIdx.x; i < e;
       i += stride) {
    uint32_t v = send_idx[i];
    uint32_t bit = v - v_begin;
    if ((chg_words[bit >> 5] >> (bit & 31)) & 1u) {
      unsigned long long pos = atomicAdd(cnt, 1ull);
      out[b + pos] = (static_cast<unsigned long long>(v) << 32) | state[v];
    }
  }
}

__global__ void mirror_scatter_pairs_kernel(
    const unsigned long long* __restrict__ pairs, uint64_t n,
    uint32_t* __restrict__ state) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride)
    state[pairs[i] >> 32] = static_cast<uint32_t>(pairs[i]);
}

static void mirror_sync_changed(GpuContext::Impl& I, TcpComm* comm,
                                DeviceGraph& g, void* state4,
                                const uint32_t* chg_words, int rank,
                                int world, hipStream_t s) {
  uint64_t ns = g.mr_send_off.back();
  uint64_t nr = g.mr_recv_off.back();
  // pair staging reuses the mirror buffers when large enough (8 B/entry;
  // recvbuf doubles as the compaction bounce, so size it for both sides)
  uint64_t big = (ns > nr ? ns : nr) * 8 + 8;
  if (g.mr_sendbuf.size() < ns * 8 + 8) g.mr_sendbuf.resize(ns * 8 + 8);
  if (g.mr_recvbuf.size() < big) g.mr_recvbuf.resize(big);
  DeviceBuffer<unsigned long long> cnts(world);
  cnts.zero(s);
  auto* pairs = reinterpret_cast<unsigned long long*>(g.mr_sendbuf.data());
  for (int q = 0; q < world; ++q) {
    uint64_t b = g.mr_send_off[q], e = g.mr_send_off[q + 1];
    if (e > b)
      mirror_pack_sparse_kernel<<<grid_for(e - b), kBlock, 0, s>>>(
          g.mr_send_idx.data(), b, e, chg_words, g.v_begin,
          static_cast<const uint32_t*>(state4), cnts.data() + q, pairs);
  }
  auto hc = cnts.download(s);
  std::vector<uint64_t> mine(world);
  for (int q = 0; q < world; ++q) mine[q] = hc[q];
  std::vector<uint64_t> matrix(static_cast<size_t>(world) * world);
  comm->allgather(mine.data(), world * 8, matrix.data());
  std::vector<uint64_t> sb(world + 1), rb(world + 1);
  sb[0] = 0;
  rb[0] = 0;
  for (int q = 0; q < world; ++q) sb[q + 1] = sb[q] + mine[q] * 8;
  uint64_t recv_pairs = 0;
  for (int p = 0; p < world; ++p) {
    uint64_t from_p =
        p == rank ? 0 : matrix[static_cast<size_t>(p) * world + rank];
    rb[p + 1] = rb[p] + from_p * 8;
    recv_pairs += from_p;
  }
  // compact the capacity regions into contiguous send order: copy each
  // peer's [b*8, b*8 + cnt*8) down — regions are already at b*8; the
  // contiguous layout needs offsets sb. D2D per peer (async, small).
  for (int q = world - 1; q >= 0; --q) {
    if (!mine[q] || g.mr_send_off[q] * 8 == sb[q]) continue;
    HIP_CHECK(hipMemcpyAsync(
        g.mr_recvbuf.data() + sb[q],
        g.mr_sendbuf.data() + g.mr_send_off[q] * 8, mine[q] * 8,
        hipMemcpyDeviceToDevice, s));
  }
  // regions that moved were staged into recvbuf — move back contiguously
  for (int q = world - 1; q >= 0; --q) {
    if (!mine[q] || g.mr_send_off[q] * 8 == sb[q]) continue;
    HIP_CHECK(hipMemcpyAsync(g.mr_sendbuf.data() + sb[q],
                             g.mr_recvbuf.data() + sb[q], mine[q] * 8,
                             hipMemcpyDeviceToDevice, s));
  }
  I.ev_pack.record(s);
  I.ev_pack.wait_on(I.comm_stream);
  I.dc.sendrecv(g.mr_sendbuf.data(), sb, g.mr_recvbuf.data(), rb,
                I.comm_stream);
  I.ev_comm.record(I.comm_stream);
  I.ev_comm.wait_on(s);
  if (recv_pairs)
    mirror_scatter_pairs_kernel<<<grid_for(recv_pairs), kBlock, 0, s>>>(
        reinterpret_cast<const unsigned long long*>(g.mr_recvbuf.data()),
        recv_pairs, static_cast<uint32_t*>(state4));
}

// old-id -> renumbered-id for API source arguments
static uint32_t map_source(DeviceGraph& g, int64_t source, hipStream_t s) {
  uint32_t v = static_cast<uint32_t>(source);
  if (!g.permuted || v >= g.perm.size()) return v;
  uint32_t out = 0;
  HIP_CHECK(hipMemcpyAsync(&out, g.perm.data() + v, 4,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return out;
}

// canonical WCC labels under renumbering: component label = min OLD id
__global__ void wcc_minold_kernel(const uint32_t* __restrict__ parent,
                                  const uint32_t* __restrict__ inv,
                                  uint32_t n, uint32_t* __restrict__ m) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n;
       v += stride)
    atomicMin(&m[parent[v]], inv[v]);
}

__global__ void wcc_relabel_kernel(const uint32_t* __restrict__ parent,
                                   const uint32_t* __restrict__ m,
                                   uint32_t v_begin, uint32_t n,
                                   uint32_t* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    out[i] = m[parent[v_begin + i]];
}

// Scheduler dispatch (reference --lb flag, default cta/cm) over a frontier
// whose degree prefix `offsets` (qn + 1 entries, `total` arcs) is already
// scanned: cm = LDS-staged owner search; wm = wave-granular register-staged
// CM; strict = perfectly edge-balanced; none = thread-per-row. Every
// frontier expansion launches from here, and only here is it counted.
template <typename Op>
void launch_expand(GpuContext::Impl& I, const DevGraphView& view,
                   const uint32_t* q, uint32_t qn, const uint64_t* offsets,
                   uint64_t total, Op op, hipStream_t s) {
  if (qn == 0) return;
  static const char* lb = getenv("GRAPEHIP_LB");
  if (lb && lb[0] == 's') {
    ++I.expand_counts[kLbStrict];
    expand_strict_frontier<Op><<<grid_for(total), kBlock, 0, s>>>(
        view, q, qn, offsets, total, op);
  } else if (lb && lb[0] == 'n') {
    ++I.expand_counts[kLbNone];
    expand_none_frontier<Op><<<grid_for(qn), kBlock, 0, s>>>(view, q, qn,
                                                             op);
  } else if (lb && lb[0] == 'w') {
    ++I.expand_counts[kLbWm];
    expand_wm_frontier<Op><<<grid_for(qn), kBlock, 0, s>>>(view, q, qn,
                                                           op);
  } else {
    ++I.expand_counts[kLbCm];
    // arcs per tile: read once per process, like GRAPEHIP_LB
    static const uint32_t tile = [] {
      const char* e = getenv("GRAPEHIP_EXPAND_TILE");
      if (!e) return kExpandTile;
      long v = atol(e);
      if (v < kBlock || v % kBlock != 0 || v > (1l << 30))
        throw std::runtime_error(
            "GRAPEHIP_EXPAND_TILE must be a multiple of 256, at least 256");
      return static_cast<uint32_t>(v);
    }();
    if (total == 0) return;  // a frontier of sinks: nothing to launch
    const uint64_t ntiles = (total + tile - 1) / tile;
    expand_cm_frontier<Op>
        <<<static_cast<int>(std::min<uint64_t>(ntiles, kMaxGrid)), kBlock, 0,
           s>>>(view, q, qn, offsets, total, tile, op);
  }
}

// Degree prefix of a frontier into foff (qn + 1 entries), through fdeg;
// returns the frontier's arc total. Grows the two buffers as needed; an
// empty frontier launches nothing and leaves them alone.
static uint64_t scan_frontier_degrees(GpuContext::Impl& I,
                                      const DevGraphView& view,
                                      const uint32_t* q, uint32_t qn,
                                      DeviceBuffer<uint32_t>& fdeg,
                                      DeviceBuffer<uint64_t>& foff,
                                      hipStream_t s) {
  if (qn == 0) return 0;
  if (fdeg.size() < qn) fdeg.resize(qn + (qn >> 2) + 64);
  if (foff.size() < qn + 1) foff.resize(qn + (qn >> 2) + 65);
  gather_deg_kernel<<<grid_for(qn), kBlock, 0, s>>>(view, q, qn,
                                                    fdeg.data());
  return exclusive_scan(fdeg.data(), foff.data(), qn, s, I.scan);
}

// generic frontier expansion helper: scan degrees, then launch_expand
template <typename Op>
void expand_frontier(GpuContext::Impl& I, const DevGraphView& view,
                     const uint32_t* q, uint32_t qn, Op op, hipStream_t s) {
  if (qn == 0) return;
  uint64_t total = scan_frontier_degrees(I, view, q, qn, I.frontier_deg,
                                         I.frontier_off, s);
  launch_expand(I, view, q, qn, I.frontier_off.data(), total, op, s);
}

// owned slice of a u32 depth array as int64, unreached = INT64_MAX
static std::vector<int64_t> fetch_depth_i64(const uint32_t* depth,
                                            const DeviceGraph& g,
                                            hipStream_t s) {
  const uint32_t owned = g.owned();
  std::vector<uint32_t> d32(owned);
  if (owned)
    HIP_CHECK(hipMemcpyAsync(d32.data(), depth + g.v_begin, owned * 4ull,
                             hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  std::vector<int64_t> out(owned);
  for (uint32_t i = 0; i < owned; ++i)
    out[i] = d32[i] == 0xFFFFFFFFu ? std::numeric_limits<int64_t>::max()
                                   : static_cast<int64_t>(d32[i]);
  return out;
}

// ---------------------------------------------------------------------------
// BFS
// ---------------------------------------------------------------------------
GpuRunResult GpuContext::bfs(DeviceGraph& g, int64_t source,
                             bool fetch) {
  RangeMarker _mk("grapehip::bfs");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  DevGraphView view = make_view(g, rank_, world_);
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  uint64_t cap = view.slice;
  bool multi = world_ > 1;

  const bool pull_capable = !g.directed || g.has_in;
  if (pull_capable) ensure_buckets(g, I, s);
  if (multi && pull_capable) ensure_mirrors(I, comm_, g, rank_, world_, s);
  const uint64_t* pull_off = !g.directed ? g.oe_off.data() : g.ie_off.data();
  const uint32_t* pull_dst = !g.directed ? g.oe_dst.data() : g.ie_dst.data();

  // context workspace, shared with sssp(): no allocation after the first
  // call on the largest graph
  size_t bm_words = (static_cast<size_t>(owned) + 31) / 32 + 1;
  grow(I.trav_state, nv_pad);
  grow(I.trav_q[0], static_cast<size_t>(owned) + 64);
  grow(I.trav_near_bm, bm_words);
  uint32_t* const depth = I.trav_state.data();
  uint32_t* const q = I.trav_q[0].data();
  uint32_t* const next_bm = I.trav_near_bm.data();
  DeviceBuffer<uint32_t>& fdeg = I.trav_fdeg;
  DeviceBuffer<uint64_t>& foff = I.trav_foff;
  const DevHalo halo = halo_reserve(
      I, world_, cap, view.slice, (static_cast<uint64_t>(nv_pad) + 31) / 32);

  RunBracket br(I, comm_);

  if (nv_pad)
    HIP_CHECK(hipMemsetAsync(depth, 0xFF, static_cast<size_t>(nv_pad) * 4, s));
  HIP_CHECK(hipMemsetAsync(next_bm, 0, bm_words * 4, s));
  if (multi) halo_reset(I, s);
  uint32_t src = map_source(g, source, s);
  if (src >= g.v_begin && src < g.v_end)
    bfs_seed_kernel<<<1, 1, 0, s>>>(depth, src, g.v_begin,
                                    next_bm);
  uint64_t global_curr = 0;
  uint32_t qn = compact_frontier_global(I, comm_, world_, next_bm, owned,
                                        g.v_begin, q, s, global_curr);
  uint32_t level = 0;
  int rounds = 0;
  // Beamer-style switch: pull when the frontier's out-edges exceed a
  // fraction of the stored edges (cuda/bfs/bfs.h heuristic, retuned).
  static const int pull_div = [] {
    const char* e = getenv("GRAPEHIP_BFS_PULL_DIV");
    return e ? atoi(e) : 16;
  }();
  const uint64_t pull_edge_threshold = g.total_edges / pull_div;
  while (global_curr > 0) {
    bool use_pull = false;
    uint64_t fedges = scan_frontier_degrees(I, view, q, qn, fdeg, foff, s);
    if (pull_capable) {
      uint64_t gedges = multi ? comm_->allreduce_sum(fedges) : fedges;
      use_pull = gedges > pull_edge_threshold;
    }
    if (use_pull) {
      if (multi) {
        // refresh referenced remote depths only (vs allgathering every
        // slice): the pull scan reads depth[dst] for local dsts alone
        mirror_sync_begin(I, g, depth, s);
        mirror_sync_end(I, g, depth, s);
      }
      DevBitmap nb{next_bm};
      if (g.n_small)
        bfs_pull_small_kernel<<<grid_for(g.n_small), kBlock, 0, s>>>(
            pull_off, pull_dst, g.rows_small.data(), g.n_small, g.v_begin,
            depth, level, nb);
      if (g.n_mid)
        bfs_pull_mid_kernel<<<grid_for(g.n_mid * kWave), kBlock, 0, s>>>(
            pull_off, pull_dst, g.rows_mid.data(), g.n_mid, g.v_begin,
            depth, level, nb);
      if (g.n_large)
        bfs_pull_large_kernel<<<static_cast<int>(std::min<uint64_t>(
                                    std::max<uint64_t>(g.n_large, 1),
                                    kMaxGrid)),
                                kBlock, 0, s>>>(
            pull_off, pull_dst, g.rows_large.data(), g.n_large, g.v_begin,
            depth, level, nb);
    } else {
      BfsOp op{depth, level + 1, DevBitmap{next_bm}, g.v_begin,
               g.v_end, multi, halo};
      launch_expand(I, view, q, qn, foff.data(), fedges, op, s);
      if (multi)
        halo_round<uint32_t>(I, comm_, rank_, world_, depth, cap,
                             BfsRecvOp{depth, DevBitmap{next_bm}, g.v_begin},
                             s);
    }
    qn = compact_frontier_global(I, comm_, world_, next_bm, owned, g.v_begin,
                                 q, s, global_curr);
    if (getenv("GRAPEHIP_DEBUG"))
      fprintf(stderr, "[bfs] level=%u mode=%s fedges=%lu next=%u t=%.1fms\n",
              level, use_pull ? "pull" : "push", (unsigned long)fedges, qn,
              br.elapsed_ms());
    ++level;
    ++rounds;
  }
  GpuRunResult res = br.finish(rounds, g.input_edges);
  if (fetch) res.i64 = fetch_depth_i64(depth, g, s);
  return res;
}

// ---------------------------------------------------------------------------
// SSSP (near-far delta stepping; cuda/sssp/sssp.h parity)
// ---------------------------------------------------------------------------
GpuRunResult GpuContext::sssp(DeviceGraph& g, int64_t source,
                              float delta, bool fetch) {
  RangeMarker _mk("grapehip::sssp");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  DevGraphView view = make_view(g, rank_, world_);
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  uint64_t cap = view.slice;
  bool multi = world_ > 1;

  // context workspace, shared with bfs(): no allocation after the first
  // call on the largest graph
  size_t own_words = (static_cast<size_t>(owned) + 31) / 32 + 1;
  uint64_t glob_words = (static_cast<uint64_t>(nv_pad) + 31) / 32;
  grow(I.trav_state, nv_pad);
  for (auto& b : I.trav_q)  // near and far queues, double-buffered
    grow(b, static_cast<size_t>(owned) + 64);
  grow(I.trav_fcnt, 2);
  grow(I.trav_near_bm, own_words);
  grow(I.trav_far_bm, glob_words);
  float* const dist = reinterpret_cast<float*>(I.trav_state.data());
  unsigned long long* const fcnt = I.trav_fcnt.data();
  uint32_t* const near_bm = I.trav_near_bm.data();
  uint32_t* const far_bm = I.trav_far_bm.data();
  DeviceBuffer<uint32_t>& fdeg = I.trav_fdeg;
  DeviceBuffer<uint64_t>& foff = I.trav_foff;
  const DevHalo halo = halo_reserve(I, world_, cap, view.slice, glob_words);
  if (delta <= 0) {
    // sweep across LiveJournal/orkut/datagen shapes put the optimum on a
    // wide plateau around 16x the mean edge weight (profiles/ r01 sweep);
    // the degree-scaled Davidson heuristic was 2x off on dense graphs.
    double mean_w = 1.0;
    if (g.weighted && g.local_edges) {
      size_t n_sample = std::min<uint64_t>(g.local_edges, 1u << 20);
      std::vector<float> h(n_sample);
      HIP_CHECK(hipMemcpyAsync(h.data(), g.oe_w.data(), n_sample * 4,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      double acc = 0;
      for (float w : h) acc += w;
      mean_w = acc / n_sample;
    }
    if (comm_ && world_ > 1)
      mean_w = comm_->allreduce_max_double(mean_w);
    delta = static_cast<float>(16.0 * mean_w);
  }

  RunBracket br(I, comm_);

  fill(dist, std::numeric_limits<float>::max(), nv_pad, s);
  HIP_CHECK(hipMemsetAsync(fcnt, 0, 2 * sizeof(unsigned long long), s));
  HIP_CHECK(hipMemsetAsync(near_bm, 0, own_words * 4, s));
  if (glob_words) HIP_CHECK(hipMemsetAsync(far_bm, 0, glob_words * 4, s));
  if (multi) halo_reset(I, s);
  uint32_t src = map_source(g, source, s);
  if (src >= g.v_begin && src < g.v_end)
    sssp_seed_kernel<<<1, 1, 0, s>>>(dist, src, g.v_begin,
                                     near_bm);
  uint32_t* nearq[2] = {I.trav_q[0].data(), I.trav_q[1].data()};
  uint32_t* farq[2] = {I.trav_q[2].data(), I.trav_q[3].data()};
  int ncur = 0, fcur = 0;
  float prio = 0.0f;
  int rounds = 0;
  unsigned long long zero = 0;
  std::vector<unsigned long long> hfc(2);
  uint64_t g_near = 0;
  uint32_t qn = compact_frontier_global(I, comm_, world_, near_bm, owned,
                                        g.v_begin, nearq[ncur], s, g_near);
  for (;;) {
    float prio_hi = prio + delta;
    uint64_t fedges = 0;
    if (qn) {
      fedges =
          scan_frontier_degrees(I, view, nearq[ncur], qn, fdeg, foff, s);
      SsspOp op{dist, prio_hi, DevBitmap{near_bm},
                DevQueue{farq[fcur], fcnt + fcur},
                DevBitmap{far_bm}, g.v_begin, g.v_end, multi, halo};
      launch_expand(I, view, nearq[ncur], qn, foff.data(), fedges, op, s);
    }
    if (multi)
      halo_round<float>(I, comm_, rank_, world_, dist, cap,
                        SsspRecvOp{dist, prio_hi, DevBitmap{near_bm},
                                   DevQueue{farq[fcur], fcnt + fcur},
                                   DevBitmap{far_bm}, g.v_begin},
                        s);
    ++rounds;
    uint32_t next_qn =
        compact_frontier_global(I, comm_, world_, near_bm, owned, g.v_begin,
                                nearq[1 - ncur], s, g_near);
    if (getenv("GRAPEHIP_DEBUG"))
      fprintf(stderr,
              "[sssp] round=%d prio=%.0f in=%u fedges=%lu next=%u t=%.1fms\n",
              rounds, prio, qn, (unsigned long)fedges, next_qn,
              br.elapsed_ms());
    ncur = 1 - ncur;
    qn = next_qn;
    if (g_near > 0) continue;
    // near exhausted globally: advance priority, repartition far buckets
    HIP_CHECK(hipMemcpyAsync(hfc.data(), fcnt, 16,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t far_n = hfc[fcur];
    uint64_t g_far = multi ? comm_->allreduce_sum(far_n) : far_n;
    if (g_far == 0) break;
    while (g_near == 0 && g_far > 0) {
      prio += delta;
      float new_hi = prio + delta;
      if (far_n)
        sssp_repart_kernel<<<grid_for(far_n), kBlock, 0, s>>>(
            farq[fcur], static_cast<uint32_t>(far_n), dist, new_hi,
            DevBitmap{near_bm}, g.v_begin,
            DevQueue{farq[1 - fcur], fcnt + (1 - fcur)},
            DevBitmap{far_bm});
      HIP_CHECK(hipMemcpyAsync(fcnt + fcur, &zero, 8,
                               hipMemcpyHostToDevice, s));
      qn = compact_frontier_global(I, comm_, world_, near_bm, owned,
                                   g.v_begin, nearq[ncur], s, g_near);
      HIP_CHECK(hipMemcpyAsync(hfc.data(), fcnt, 16,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      fcur = 1 - fcur;
      far_n = hfc[fcur];
      g_far = multi ? comm_->allreduce_sum(far_n) : far_n;
    }
    if (g_near == 0 && g_far == 0) break;
  }
  GpuRunResult res = br.finish(rounds, g.input_edges);
  if (fetch) {
    std::vector<float> d32(owned);
    HIP_CHECK(hipMemcpyAsync(d32.data(), dist + g.v_begin, owned * 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    res.f64.resize(owned);
    for (uint32_t i = 0; i < owned; ++i)
      res.f64[i] = d32[i] >= std::numeric_limits<float>::max()
                       ? std::numeric_limits<double>::max()
                       : static_cast<double>(d32[i]);
  }
  return res;
}

// ---------------------------------------------------------------------------
// PageRank (push + fp64 hw atomics; reduce-scatter/allgather over xGMI)
// ---------------------------------------------------------------------------

// The id-segment pull of one iteration: item counters to zero, then the
// persistent kernel at the arc depth in effect. The reduce follows it.
static void launch_pr_pull_seg(DeviceGraph& g, GpuContext::Impl& I,
                               const uint32_t* pull_dst, const float* contrib,
                               hipStream_t s) {
  g.seg_ctr.zero(s);
  const int grid = I.num_cus * kPrSegBlocksPerCu;
  auto pull_seg = [&](auto depth) {
    constexpr int D = decltype(depth)::value;
    if (pr_seg_knobs().nt)
      pr_pull_seg_kernel<true, D><<<grid, kBlock, 0, s>>>(
          g.seg_view, pull_dst, contrib, g.seg_ctr.data(), g.seg_part.data());
    else
      pr_pull_seg_kernel<false, D><<<grid, kBlock, 0, s>>>(
          g.seg_view, pull_dst, contrib, g.seg_ctr.data(), g.seg_part.data());
  };
  switch (arc_depth()) {
    case 4: pull_seg(std::integral_constant<int, 4>{}); break;
    case 2: pull_seg(std::integral_constant<int, 2>{}); break;
    default: pull_seg(std::integral_constant<int, 1>{});
  }
}

// The epilogue path: pull direction, single GPU, not tiled, undirected,
// tol <= 0, iters >= 1 (pagerank() decides). Against the fused path it
// drops, per iteration, the acc round trip, pr_fused_apply_kernel, nine of
// ten rank writes and the dangling pair's memset, atomics and copy; per
// call, the fills of rank and acc and the passes over all owned rows that
// found the dangling sum and the first contributions. The sums, their
// order and the fp64 expressions are the fused path's; only the first
// dangling value differs, n * (1/N) instead of an atomic sum of n copies
// of 1/N.
GpuRunResult GpuContext::pagerank_epilogue(DeviceGraph& g, double damping,
                                           int iters, bool seg, bool fetch) {
  auto& I = *impl_;
  hipStream_t s = I.compute;
  const uint32_t nv_pad = padded_nv(g, world_);
  const uint32_t owned = g.owned();
  const double inv_n = 1.0 / static_cast<double>(g.nv_real);
  const double n_iso = static_cast<double>(g.n_isolated_real);
  const uint64_t* off = g.oe_off.data();
  const uint32_t* dst = g.oe_dst.data();
  ++I.pr_epi_counts[0];

  // on the DeviceGraph: the captured hipGraphs bake these pointers
  if (g.pr_contrib2.size() < nv_pad) g.pr_contrib2.resize(nv_pad);
  if (g.pr_epi_scal.size() < 3) g.pr_epi_scal.resize(3);
  float* const buf[2] = {g.pr_contrib.data(), g.pr_contrib2.data()};
  double* const sc = g.pr_epi_scal.data();
  double* const rank = g.pr_rank.data();

  RunBracket br(I, comm_);

  // Every owned row's rank is written below: the active rows' by the last
  // iteration, the others' by pr_fill_isolated_kernel. The rows of the
  // buffer outside the owned range keep the 1/N that the fused path's fill
  // leaves there.
  fill(rank, inv_n, g.v_begin, s);
  fill(rank + g.v_begin + owned, inv_n, nv_pad - g.v_begin - owned, s);
  pr_epi_init_kernel<<<1, 1, 0, s>>>(sc, n_iso * inv_n, inv_n);
  if (g.n_active)
    pr_epi_contrib0_kernel<<<grid_for(g.n_active), kBlock, 0, s>>>(
        g.rows_active.data(), g.n_active, off, inv_n, g.v_begin, buf[0]);

  // one iteration: the scalar step, then the pulls with their epilogues
  auto iteration = [&](const float* cin, float* cout, bool last) {
    pr_epi_scalar_kernel<<<1, 1, 0, s>>>(sc, inv_n, damping, n_iso);
    const PrEpilogue ep{sc + 1, damping, cout, rank};
    auto launch = [&](auto tag) {
      constexpr int E = decltype(tag)::value;
      if (g.n_small)
        pr_pull_small_cm_kernel<0, E>
            <<<grid_for(g.n_small), kBlock, 0, s>>>(
                off, dst, cin, g.rows_small.data(), g.n_small, g.v_begin,
                g.v_begin, g.v_end, nullptr, ep);
      if (seg) {
        launch_pr_pull_seg(g, I, dst, cin, s);
        pr_seg_reduce_kernel<E><<<grid_for(g.n_seg_rows), kBlock, 0, s>>>(
            g.seg_rows.data(), g.seg_row_first.data(), g.n_seg_rows,
            g.seg_part.data(), g.v_begin, nullptr, g.seg_row_deg.data(), ep);
      }
    };
    if (last) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 1>{});
  };

  // Iterations but the last: captured once per (graph, damping) as two
  // hipGraphs, buf[0] -> buf[1] and back, and replayed alternately; as for
  // the fused path, a graph's first call records them on the stream
  // instead. The last iteration, which writes rank, is always recorded.
  const bool capture = g.pr_calls++ > 0 && iters > 1;
  hipGraphExec_t exec[2] = {
      reinterpret_cast<hipGraphExec_t>(g.pr_epi_exec[0]),
      reinterpret_cast<hipGraphExec_t>(g.pr_epi_exec[1])};
  if (capture && (!exec[0] || g.pr_epi_damping != damping)) {
    for (int k = 0; k < 2; ++k) {
      if (exec[k]) HIP_CHECK(hipGraphExecDestroy(exec[k]));
      exec[k] = nullptr;
      g.pr_epi_exec[k] = nullptr;
    }
    for (int k = 0; k < 2; ++k) {
      hipGraph_t graph = nullptr;
      HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      iteration(buf[k], buf[k ^ 1], false);
      HIP_CHECK(hipStreamEndCapture(s, &graph));
      HIP_CHECK(hipGraphInstantiate(&exec[k], graph, nullptr, nullptr, 0));
      HIP_CHECK(hipGraphDestroy(graph));
      g.pr_epi_exec[k] = exec[k];
    }
    g.pr_epi_damping = damping;
  }

  for (int it = 0; it + 1 < iters; ++it) {
    if (capture) {
      HIP_CHECK(hipGraphLaunch(exec[it & 1], s));
      ++I.pr_epi_counts[1];
    } else {
      iteration(buf[it & 1], buf[(it & 1) ^ 1], false);
    }
  }
  iteration(buf[(iters - 1) & 1], buf[iters & 1], true);
  pr_fill_isolated_kernel<<<grid_for(owned), kBlock, 0, s>>>(
      g.active_bm.data(), owned, g.v_begin, sc + 2, rank);

  GpuRunResult res =
      br.finish(iters, static_cast<uint64_t>(iters) * g.total_edges);
  if (fetch) {
    res.f64.resize(owned);
    HIP_CHECK(hipMemcpyAsync(res.f64.data(), rank + g.v_begin,
                             static_cast<size_t>(owned) * 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  return res;
}

GpuRunResult GpuContext::pagerank(DeviceGraph& g, double damping,
                                  int iters, double tol, bool fetch) {
  RangeMarker _mk("grapehip::pagerank");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  uint32_t slice = g.seg_host.size() > 1 ? g.seg_host[1] - g.seg_host[0]
                                         : g.nv_global;
  bool multi = world_ > 1;
  const double N = static_cast<double>(g.nv_real);

  // pull path: undirected symmetric storage (out-CSR == neighborhood) or
  // directed with an in-CSR. Fallback: fp64-atomic push.
  const bool pull = !g.directed || g.has_in;
  const uint64_t* pull_off =
      (!g.directed ? g.oe_off.data() : g.ie_off.data());
  const uint32_t* pull_dst =
      (!g.directed ? g.oe_dst.data() : g.ie_dst.data());
  if (pull) ensure_buckets(g, I, s);
  if (pull && multi) ensure_mirrors(I, comm_, g, rank_, world_, s);
  // dst-tiled pull stream: auto-selected by density. On sparse shapes
  // (datagen mean degree ~5) the short per-src runs mean one fp64 L2
  // atomic per edge (~40 G/s cap) and the row pull wins ~3x; on dense
  // shapes (orkut mean degree ~142) runs amortize the atomics and the
  // tiled stream wins ~8% (same-box A/B: 46.3 vs 50.3 ms).
  // GRAPEHIP_PR_TILED={0,1} overrides.
  uint64_t pull_edges = !g.directed ? g.oe_dst.size() : g.ie_dst.size();
  double mean_pull_deg =
      g.owned_real ? static_cast<double>(pull_edges) / g.owned_real : 0.0;
  const char* te = getenv("GRAPEHIP_PR_TILED");
  const bool want_tiled =
      pull && (te ? atoi(te) != 0 : mean_pull_deg >= 64.0);
  if (want_tiled) ensure_pr_tiles(g, *impl_, s);
  const bool tiled = want_tiled && g.pr_ntiles > 0;
  // id-segment pull for the mid and hub rows: single-GPU row pull only
  const bool seg = pull && !multi && !tiled && ensure_pr_segments(g, I, s);
  if (pull && !multi && !tiled) ++I.pr_path_counts[seg ? 0 : 1];

  // working set lives on the DeviceGraph: the cached hipGraph bakes these
  // pointers (locals would dangle across calls — GPU fault under realloc)
  if (g.pr_rank.size() < nv_pad) {
    g.pr_rank.resize(nv_pad);
    g.pr_contrib.resize(nv_pad);
    g.pr_dangling.resize(3);
  }
  // Epilogue path (KERNELS.md "PageRank epilogues"): the pulls apply their
  // row sums themselves. It has the small and the id-segment pull; a graph
  // whose mid and hub rows go through the row-tier pulls stays on the fused
  // path, as do directed graphs and tol > 0.
  if (pr_epilogue_on() && pull && !multi && !tiled && !g.directed &&
      tol <= 0 && iters >= 1 && (seg || (!g.n_mid && !g.n_large)))
    return pagerank_epilogue(g, damping, iters, seg, fetch);
  // no sum goes through acc on the epilogue path: allocated here only
  if (g.pr_acc.size() < nv_pad) g.pr_acc.resize(nv_pad);
  DeviceBuffer<double>& rank_arr = g.pr_rank;
  DeviceBuffer<double>& acc = g.pr_acc;
  DeviceBuffer<float>& contrib = g.pr_contrib;
  DeviceBuffer<double>& d_dangling = g.pr_dangling;
  // [0]=cur, [1]=next, [2]=previous base (isolated rows' closed form)
  if (d_dangling.size() < 3) d_dangling.resize(3);
  DeviceBuffer<double> d_l1(tol > 0 ? 1 : 0);
  DevGraphView view = make_view(g, rank_, world_);

  RunBracket br(I, comm_);

  fill(rank_arr.data(), 1.0 / N, nv_pad, s);
  // Rows without a pull edge are in no bucket, so the row pulls never write
  // their acc, yet it is read for rows that have out-edges only (directed)
  // and by the multi-GPU apply over all owned rows. The buffer is shared
  // with the tiled and push paths; clear it once per call.
  if (pull && !tiled) acc.zero(s);
  int rounds = 0;
  const double inv_n = 1.0 / N;

  // phase-dispatched pull sweep (PHASE 0 whole row / 1 owned span / 2 rest)
  auto pulls = [&](int phase) {
    auto launch = [&](auto tag) {
      constexpr int P = decltype(tag)::value;
      if (g.n_small)
        pr_pull_small_cm_kernel<P><<<grid_for(g.n_small), kBlock, 0, s>>>(
            pull_off, pull_dst, contrib.data(), g.rows_small.data(),
            g.n_small, g.v_begin, g.v_begin, g.v_end, acc.data(),
            PrEpilogue{});
      if (seg) {
        // P == 0 here. Every partial is stored by the pull and read by the
        // reduce; the kernel boundary carries them across the XCDs.
        launch_pr_pull_seg(g, I, pull_dst, contrib.data(), s);
        pr_seg_reduce_kernel<0><<<grid_for(g.n_seg_rows), kBlock, 0, s>>>(
            g.seg_rows.data(), g.seg_row_first.data(), g.n_seg_rows,
            g.seg_part.data(), g.v_begin, acc.data(), nullptr, PrEpilogue{});
        return;
      }
      if (g.n_mid)
        pr_pull_mid_kernel<P><<<grid_for(g.n_mid * kWave), kBlock, 0, s>>>(
            pull_off, pull_dst, contrib.data(), g.rows_mid.data(), g.n_mid,
            g.v_begin, g.v_begin, g.v_end, acc.data());
      if (g.n_large) {
        pr_pull_large_kernel<P><<<std::min<uint64_t>(g.n_hub_items, kMaxGrid),
                                  kBlock, 0, s>>>(
            pull_off, pull_dst, contrib.data(), g.rows_large.data(),
            g.hub_item_row.data(), g.hub_item_seg.data(), g.n_hub_items,
            g.v_begin, g.v_end, g.pr_hub_part.data());
        pr_hub_reduce_kernel<P><<<grid_for(g.n_large * kWave), kBlock, 0,
                                  s>>>(
            g.rows_large.data(), g.hub_row_first.data(), g.n_large,
            g.pr_hub_part.data(), g.v_begin, acc.data());
      }
    };
    if (phase == 0) launch(std::integral_constant<int, 0>{});
    else if (phase == 1) launch(std::integral_constant<int, 1>{});
    else launch(std::integral_constant<int, 2>{});
  };
  // fold the global dangling sum on the host via the pinned scalar
  // (the D2H was enqueued earlier; ev_scal gates only that copy, so the
  // GPU keeps crunching whatever was launched after it)
  auto fold_dangling = [&]() {
    I.ev_scal.sync();
    std::vector<double> all(world_);
    comm_->allgather(I.h_scal, 8, all.data());
    double dang = 0;
    for (double x : all) dang += x;
    I.h_scal[1] = dang;
    HIP_CHECK(hipMemcpyAsync(d_dangling.data(), I.h_scal + 1, 8,
                             hipMemcpyHostToDevice, s));
  };

  // Single-GPU pull path: the fused iteration folds apply + the NEXT
  // iteration's contrib/dangling into one rank pass (bootstrap computes
  // the first dangling/contrib outside the loop); the dangling scalar
  // ping-pongs through a fixed [cur,next] pair so the sequence is
  // hipGraph-capturable with stable pointers.
  const bool fused = pull && !multi;
  auto fused_bootstrap = [&]() {
    d_dangling.zero(s);
    fill(d_dangling.data() + 2, inv_n, 1, s);  // isolated rows start at 1/N
    pr_dangling_kernel<<<grid_for(g.owned_real), kBlock, 0, s>>>(
        rank_arr.data(), g.oe_off.data(), g.owned_real, g.v_begin,
        d_dangling.data());
    pr_contrib_kernel<<<grid_for(g.owned_real), kBlock, 0, s>>>(
        rank_arr.data(), g.oe_off.data(), g.owned_real, g.v_begin,
        contrib.data() + g.v_begin);
  };
  auto fused_iteration = [&]() {
    if (tiled) {
      acc.zero(s);
      static int tile_grid_f = [] {
        const char* e = getenv("GRAPEHIP_PR_GRID");
        return e ? atoi(e) : 8192;
      }();
      if (g.pr_total)
        pr_tiled_pull_kernel<<<tile_grid_f, kBlock, 0, s>>>(
            g.pr_tiles.data(), 0, g.pr_total, contrib.data(), acc.data());
    } else {
      pulls(0);
    }
    HIP_CHECK(hipMemsetAsync(d_dangling.data() + 1, 0, 8, s));
    if (tol > 0) d_l1.zero(s);
    pr_fused_apply_kernel<<<grid_for(g.n_active), kBlock, 0, s>>>(
        rank_arr.data(), acc.data(), d_dangling.data(), inv_n, damping,
        g.v_begin, g.rows_active.data(), g.n_active, g.owned_real,
        static_cast<double>(g.n_isolated_real), d_dangling.data() + 2,
        g.oe_off.data(), contrib.data() + g.v_begin, d_dangling.data() + 1,
        tol > 0 ? d_l1.data() : nullptr);
    HIP_CHECK(hipMemcpyAsync(d_dangling.data(), d_dangling.data() + 1, 8,
                             hipMemcpyDeviceToDevice, s));
  };

  // one iteration, recorded as a stream of kernels. Single-GPU fixed-iter
  // runs capture it into a hipGraph once and replay (the iteration is
  // fully device-side: the dangling sum feeds pr_apply through a device
  // scalar). Multi-GPU pull runs overlap compute with communication: the
  // owned-span pull (phase 1) executes on the compute stream WHILE the
  // mirror exchange of remote contribs rides the comm stream over xGMI
  // and the host folds the dangling scalar — then phase 2 accumulates
  // the remote spans (north-star overlap; ROADMAP r01 design, landed).
  auto record_iteration = [&]() {
    d_dangling.zero(s);
    pr_dangling_kernel<<<grid_for(g.owned_real), kBlock, 0, s>>>(
        rank_arr.data(), g.oe_off.data(), g.owned_real, g.v_begin,
        d_dangling.data());
    if (multi) {
      HIP_CHECK(hipMemcpyAsync(I.h_scal, d_dangling.data(), 8,
                               hipMemcpyDeviceToHost, s));
      I.ev_scal.record(s);
    }
    pr_contrib_kernel<<<grid_for(g.owned_real), kBlock, 0, s>>>(
        rank_arr.data(), g.oe_off.data(), g.owned_real, g.v_begin,
        contrib.data() + g.v_begin);
    if (pull && tiled) {
      // tiled pull: edge stream grouped by dst tile (L2-hot gathers);
      // accumulates, so clear acc first. Phase A sweeps the tiles whose
      // dsts lie in the owned slice while the mirror exchange runs.
      acc.zero(s);
      static int tile_grid = [] {
        const char* e = getenv("GRAPEHIP_PR_GRID");
        return e ? atoi(e) : 8192;
      }();
      if (multi) {
        mirror_sync_begin(I, g, contrib.data(), s);
        if (g.pr_own_hi > g.pr_own_lo)
          pr_tiled_pull_kernel<<<tile_grid, kBlock, 0, s>>>(
              g.pr_tiles.data(), g.pr_own_lo, g.pr_own_hi, contrib.data(),
              acc.data());
        fold_dangling();
        mirror_sync_end(I, g, contrib.data(), s);
        if (g.pr_own_lo > 0)
          pr_tiled_pull_kernel<<<tile_grid, kBlock, 0, s>>>(
              g.pr_tiles.data(), 0, g.pr_own_lo, contrib.data(),
              acc.data());
        if (g.pr_total > g.pr_own_hi)
          pr_tiled_pull_kernel<<<tile_grid, kBlock, 0, s>>>(
              g.pr_tiles.data(), g.pr_own_hi, g.pr_total, contrib.data(),
              acc.data());
      } else {
        if (g.pr_total)
          pr_tiled_pull_kernel<<<tile_grid, kBlock, 0, s>>>(
              g.pr_tiles.data(), 0, g.pr_total, contrib.data(),
              acc.data());
      }
    } else if (pull) {
      if (multi) {
        mirror_sync_begin(I, g, contrib.data(), s);
        pulls(1);          // owned spans, overlapped with the exchange
        fold_dangling();   // host work, overlapped too
        mirror_sync_end(I, g, contrib.data(), s);
        pulls(2);          // remote spans once payloads landed
      } else {
        pulls(0);
      }
    } else {
      if (multi) fold_dangling();
      acc.zero(s);
      int nchunks = static_cast<int>((owned + kBlock - 1) / kBlock);
      expand_cm_range<false, PrPushOp>
          <<<std::min(nchunks, kMaxGrid), kBlock, 0, s>>>(
              view, PrPushOp{contrib.data() + g.v_begin, acc.data(),
                             g.v_begin});
      if (multi) I.dc.reduce_scatter_sum_f64(acc.data(), slice, s);
    }
    if (tol > 0) d_l1.zero(s);
    pr_apply_kernel<<<grid_for(owned), kBlock, 0, s>>>(
        rank_arr.data(), acc.data(), d_dangling.data(), inv_n, damping,
        g.v_begin, owned, tol > 0 ? d_l1.data() : nullptr);
  };

  // capture once per graph (cached on the DeviceGraph: the instantiate
  // cost would otherwise swamp small runs; warmup absorbs it)
  const bool capture = !multi && tol <= 0 && g.pr_calls++ > 0;
  hipGraphExec_t graph_exec =
      reinterpret_cast<hipGraphExec_t>(g.pr_graph_exec);
  if (fused) fused_bootstrap();
  if (capture && (!graph_exec || g.pr_graph_damping != damping)) {
    if (graph_exec) {
      HIP_CHECK(hipGraphExecDestroy(graph_exec));
      graph_exec = nullptr;
    }
    hipGraph_t graph = nullptr;
    HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    if (fused) fused_iteration();
    else record_iteration();
    HIP_CHECK(hipStreamEndCapture(s, &graph));
    HIP_CHECK(hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphDestroy(graph));
    g.pr_graph_exec = graph_exec;
    g.pr_graph_damping = damping;
  }

  for (int it = 0; it < iters; ++it) {
    if (capture)
      HIP_CHECK(hipGraphLaunch(graph_exec, s));
    else if (fused)
      fused_iteration();
    else
      record_iteration();
    ++rounds;
    if (tol > 0) {
      // competitor-equivalent convergence (reference pagerank_local.h):
      // stop when the global L1 delta drops under tol
      double l1 = 0;
      HIP_CHECK(hipMemcpyAsync(&l1, d_l1.data(), 8, hipMemcpyDeviceToHost,
                               s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (multi) {
        std::vector<double> all(world_);
        comm_->allgather(&l1, 8, all.data());
        l1 = 0;
        for (double x : all) l1 += x;
      }
      if (l1 < tol) break;
    }
  }
  // the fused iterations left the isolated rows to the scalar recurrence;
  // complete the device-resident result (outside the captured graph)
  if (fused)
    pr_fill_isolated_kernel<<<grid_for(owned), kBlock, 0, s>>>(
        g.active_bm.data(), owned, g.v_begin, d_dangling.data() + 2,
        rank_arr.data());
  GpuRunResult res =
      br.finish(rounds, static_cast<uint64_t>(iters) * g.total_edges);
  if (fetch) {
    res.f64.resize(owned);
    HIP_CHECK(hipMemcpyAsync(res.f64.data(), rank_arr.data() + g.v_begin,
                             owned * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  return res;
}

// ---------------------------------------------------------------------------
// WCC (min-root union-find, replicated parent + allreduce-min merge)
// ---------------------------------------------------------------------------
GpuRunResult GpuContext::wcc(DeviceGraph& g, bool fetch) {
  RangeMarker _mk("grapehip::wcc");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  DevGraphView view = make_view(g, rank_, world_);
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  bool multi = world_ > 1;
  // Directed graphs: the Afforest giant-skip is only sound when every
  // vertex can see all edges that touch it. An edge u->v stored solely in
  // a skipped giant row u may be the ONLY link to v — with an in-CSR the
  // rest pass co-expands v's in-edges to cover it; without one the skip
  // is disabled (full fixpoint passes).
  const bool rest_use_in = g.directed && g.has_in;
  DevGraphView view_in = view;
  if (rest_use_in) {
    view_in.oe_off = g.ie_off.data();
    view_in.oe_dst = g.ie_dst.data();
    view_in.oe_w = nullptr;
  }

  DeviceBuffer<uint32_t> parent(nv_pad);
  DeviceBuffer<int> d_changed(1);
  // multi-GPU sparse-merge scratch: entries hooked this round
  size_t chg_words = (static_cast<size_t>(nv_pad) + 31) / 32;
  DeviceBuffer<uint32_t> chg_bm(multi ? chg_words : 1);
  DeviceBuffer<uint32_t> chg_q;
  DeviceBuffer<uint32_t> pairs_all;

  RunBracket br(I, comm_);

  iota_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(parent.data(), 0, nv_pad);
  if (multi) chg_bm.zero(s);
  int rounds = 0;
  constexpr int kSample = 2;
  uint32_t* marks = multi ? chg_bm.data() : nullptr;
  // scratch for the remaining-rows frontier
  DeviceBuffer<uint32_t> rest_bm((owned + 31) / 32 + 1);
  DeviceBuffer<uint32_t> rest_q(owned ? owned : 1);
  rest_bm.zero(s);
  for (;;) {
    int local_changed_any = 0;
    // 1) Afforest sampling: hook edge i per row in pass i, compressing
    //    between passes (linking via compressed roots collapses the giant
    //    component far better than hooking both edges in one pass)
    d_changed.zero(s);
    for (int which = 0; which < kSample; ++which) {
      if (owned)
        wcc_sample_kernel<<<grid_for(owned), kBlock, 0, s>>>(
            view, which, parent.data(), d_changed.data(), marks);
      wcc_compress_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(parent.data(),
                                                              nv_pad);
    }
    ++rounds;
    if (multi) {
      int ch0 = 0;
      HIP_CHECK(hipMemcpyAsync(&ch0, d_changed.data(), 4,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (ch0) local_changed_any = 1;
    }
    // 2) identify the giant component from a small host probe
    uint32_t giant = 0;
    {
      const int kProbe = 509;
      std::vector<uint32_t> roots(kProbe);
      uint32_t step = nv_pad / kProbe ? nv_pad / kProbe : 1;
      for (int i = 0; i < kProbe; ++i)
        HIP_CHECK(hipMemcpyAsync(
            &roots[i],
            parent.data() + (static_cast<uint64_t>(i) * step) % nv_pad, 4,
            hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      std::unordered_map<uint32_t, int> freq;
      int best = 0;
      for (uint32_t r : roots) {
        int c = ++freq[r];
        if (c > best) {
          best = c;
          giant = r;
        }
      }
    }
    if (g.directed && !g.has_in) giant = 0xFFFFFFFFu;  // skip unsound
    // 3) full pass restricted to rows outside the giant component,
    //    repeated to the local fixpoint
    for (;;) {
      rest_bm.zero(s);
      if (owned) {
        wcc_mark_rest_kernel<<<grid_for(owned), kBlock, 0, s>>>(
            parent.data(), view.oe_off, owned, g.v_begin, giant,
            DevBitmap{rest_bm.data()});
        if (rest_use_in)
          wcc_mark_rest_kernel<<<grid_for(owned), kBlock, 0, s>>>(
              parent.data(), view_in.oe_off, owned, g.v_begin, giant,
              DevBitmap{rest_bm.data()});
      }
      uint64_t nrest = compact_frontier(I, rest_bm.data(), owned, g.v_begin,
                                        rest_q.data(), s);
      if (nrest == 0) break;
      d_changed.zero(s);
      expand_frontier(I, view, rest_q.data(), static_cast<uint32_t>(nrest),
                      WccOp{parent.data(), d_changed.data(), marks}, s);
      if (rest_use_in)
        expand_frontier(I, view_in, rest_q.data(),
                        static_cast<uint32_t>(nrest),
                        WccOp{parent.data(), d_changed.data(), marks}, s);
      int ch = 0;
      HIP_CHECK(hipMemcpyAsync(&ch, d_changed.data(), 4,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      wcc_compress_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(parent.data(),
                                                              nv_pad);
      ++rounds;
      if (!ch) break;
      local_changed_any = 1;
    }
    if (!multi) break;
    bool any = comm_->allreduce_or(local_changed_any != 0);
    // sparse merge: ship only (entry, parent) pairs hooked this round,
    // broadcast to every peer (hooks target arbitrary global entries so
    // all ranks need them); the full allreduce-min is kept as the dense
    // fallback for churn-heavy early rounds. Compression shortcuts are
    // derived state and need no exchange — chains stay valid, and the
    // final merge below restores exact agreement (VERDICT r01 item 2:
    // per-round volume now scales with hook count, not V*world).
    {
      if (I.frontier_deg.size() < chg_words)
        I.frontier_deg.resize(chg_words + (chg_words >> 2) + 64);
      if (I.frontier_off.size() < chg_words + 1)
        I.frontier_off.resize(chg_words + (chg_words >> 2) + 65);
      popc_words_kernel<<<grid_for(chg_words), kBlock, 0, s>>>(
          chg_bm.data(), chg_words, I.frontier_deg.data());
      uint64_t nchg = exclusive_scan(I.frontier_deg.data(),
                                     I.frontier_off.data(), chg_words, s,
                                     I.scan);
      std::vector<uint64_t> counts(world_);
      comm_->allgather(&nchg, 8, counts.data());
      uint64_t total_pairs = 0;
      for (uint64_t c : counts) total_pairs += c;
      if (total_pairs * 2 >= nv_pad) {
        chg_bm.zero(s);
        I.dc.allreduce_min_u32(parent.data(), nv_pad, s);
      } else if (total_pairs) {
        std::vector<uint64_t> region(world_ + 1, 0);
        for (int f = 0; f < world_; ++f)
          region[f + 1] = region[f] + counts[f];
        if (chg_q.size() < nchg) chg_q.resize(nchg + 64);
        if (pairs_all.size() < total_pairs * 2)
          pairs_all.resize(total_pairs * 2 + 64);
        if (nchg) {
          fill_frontier_kernel<<<grid_for(chg_words), kBlock, 0, s>>>(
              chg_bm.data(), chg_words, I.frontier_off.data(), 0,
              chg_q.data());
          wcc_pack_pairs_kernel<<<grid_for(nchg), kBlock, 0, s>>>(
              chg_q.data(), nchg, parent.data(),
              pairs_all.data() + region[rank_] * 2);
        }
        std::vector<uint64_t> region_u32(world_ + 1);
        for (int f = 0; f <= world_; ++f) region_u32[f] = region[f] * 2;
        I.dc.bcast_regions_u32(pairs_all.data(), region_u32, s);
        wcc_apply_pairs_kernel<<<grid_for(total_pairs), kBlock, 0, s>>>(
            pairs_all.data(), total_pairs, region[rank_],
            region[rank_ + 1], parent.data());
      }
    }
    wcc_compress_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(parent.data(),
                                                            nv_pad);
    HIP_CHECK(hipStreamSynchronize(s));
    if (!any) break;
  }
  // exact labels for output. Multi: one dense merge first so ranks agree.
  // All paths: compress to the FIXPOINT — the loop can exit via
  // nrest==0 with entries still multiple hops from their root (path
  // halving races decide which), and the fetch below reads parent raw.
  if (multi) I.dc.allreduce_min_u32(parent.data(), nv_pad, s);
  {
    int passes = 0;
    for (;;) {
      d_changed.zero(s);
      wcc_finalize_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(
          parent.data(), nv_pad, d_changed.data());
      ++passes;
      int ch = 0;
      HIP_CHECK(hipMemcpyAsync(&ch, d_changed.data(), 4,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (!ch) break;
    }
    if (getenv("GRAPEHIP_DEBUG"))
      fprintf(stderr, "[wcc] output fixpoint passes=%d rounds=%d\n", passes,
              rounds);
  }
  GpuRunResult res = br.finish(rounds, g.input_edges);
  if (fetch) {
    std::vector<uint32_t> lab(owned);
    const uint32_t* lab_src = parent.data() + g.v_begin;
    DeviceBuffer<uint32_t> relab;
    if (g.permuted) {
      // canonical labels = component min OLD id (oracle/LDBC convention)
      DeviceBuffer<uint32_t> mo(nv_pad);
      mo.fill_bytes(0xFF, s);
      wcc_minold_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(
          parent.data(), g.inv.data(), nv_pad, mo.data());
      relab.resize(owned);
      wcc_relabel_kernel<<<grid_for(owned), kBlock, 0, s>>>(
          parent.data(), mo.data(), g.v_begin, owned, relab.data());
      lab_src = relab.data();
    }
    HIP_CHECK(hipMemcpyAsync(lab.data(), lab_src, owned * 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    res.i64.assign(lab.begin(), lab.end());
  }
  return res;
}

// ---------------------------------------------------------------------------
// CDLP (synchronous label propagation; reference examples/analytical_apps/
// cuda/cdlp/cdlp.h). MI355X design: instead of the reference's CUB segmented
// radix sort per adjacency (cuda/cdlp/cdlp.h:199-251), the label mode is
// computed with degree-tiered counting:
//   * deg <= 16:      thread-per-row, labels in registers
//   * deg <= 64:      wave-per-row ballot mode (no memory traffic at all —
//                     the wave votes labels off with __ballot/popcount)
//   * deg <= 512:     wave-per-row open-addressing hash in LDS, 4 rows per
//                     block (1024 slots x (label,count) each)
//   * deg <= 4096:    block-per-row open-addressing hash in LDS (64 KB:
//                     8192 slots x (label,count)), LDS atomics
//   * heavier rows:   block-per-row global-memory hash (L2 atomics), table
//                     space carved from one scratch pool by prefix sum
// The tiers come from the shared row partitioner; LCC's neighbor dedup runs
// over the same tiers (minus the first) with the same row decoder.
// Labels are u32 global vids (identity oids); each iteration refreshes the
// replicated label array with an in-place ncclAllGather over xGMI (the
// dense analogue of the reference's SendMsgThroughOEdges label push).
// Directed graphs use the in+out multiset (both CSRs), like the CPU app.
// ---------------------------------------------------------------------------

// --- pieces shared with LCC's dedup tiers: bounds, row decoder, hash -------

constexpr uint32_t kTierTinyDeg = 16;      // thread-per-row register tier
constexpr uint32_t kTierSmallDeg = 64;     // wave-ballot tier bound
constexpr uint32_t kTierWaveSlots = 1024;  // wave-hash tier (4 rows/block)
constexpr uint32_t kTierWaveDeg = kTierWaveSlots / 2;
constexpr uint32_t kTierMidSlots = 8192;   // block-per-row LDS table
constexpr uint32_t kTierMidDeg = kTierMidSlots / 2;  // load factor <= 0.5
constexpr uint32_t kSlotEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t slot_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// row r of the combined (off1 [+ off2]) adjacency, decoded; Len is u32
// except in the large tier
template <typename Len>
struct AdjRow {
  uint32_t v;
  uint64_t b1, b2;
  Len d1, deg;
  __device__ __forceinline__ uint32_t at(const uint32_t* __restrict__ dst1,
                                         const uint32_t* __restrict__ dst2,
                                         Len k) const {
    return k < d1 ? dst1[b1 + k] : dst2[b2 + (k - d1)];
  }
};

template <typename Len>
__device__ __forceinline__ AdjRow<Len> adj_row(
    const uint64_t* __restrict__ off1, const uint64_t* __restrict__ off2,
    uint32_t r, uint32_t v_begin) {
  AdjRow<Len> row;
  row.v = v_begin + r;
  row.b1 = off1[r];
  row.d1 = static_cast<Len>(off1[r + 1] - row.b1);
  row.deg = row.d1;
  row.b2 = 0;
  if (off2) {
    row.b2 = off2[r];
    row.deg += static_cast<Len>(off2[r + 1] - row.b2);
  }
  return row;
}

// LDS table size for a row: pow2 >= 2*deg, clamped to the tier's slots
__device__ __forceinline__ uint32_t lds_table_cap(uint32_t deg,
                                                  uint32_t slots) {
  uint32_t cap = 64;
  while (cap < 2 * deg) cap <<= 1;
  return cap > slots ? slots : cap;
}

// Tiers by combined degree, lists in degree order: tiny, small, wave, mid,
// large. The tiny tier is CDLP's; without it those rows are small rows.
struct CombinedDegTiers {
  static constexpr int kLists = 5, kBins = 5;
  const uint64_t* __restrict__ off1;
  const uint64_t* __restrict__ off2;
  bool tiny;
  __device__ __forceinline__ int operator()(uint32_t r) const {
    uint64_t deg = adj_row<uint64_t>(off1, off2, r, 0).deg;
    if (deg <= kTierSmallDeg) return tiny && deg <= kTierTinyDeg ? 0 : 1;
    return deg <= kTierWaveDeg ? 2 : (deg <= kTierMidDeg ? 3 : 4);
  }
};

// per-large-row global table capacity (pow2 >= 2*deg)
__global__ void heavy_cap_kernel(const uint64_t* __restrict__ off1,
                                 const uint64_t* __restrict__ off2,
                                 const uint32_t* __restrict__ rows,
                                 uint64_t nrows, uint32_t* __restrict__ caps) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint64_t deg = adj_row<uint64_t>(off1, off2, rows[i], 0).deg;
    uint64_t cap = 1024;
    while (cap < 2 * deg) cap <<= 1;
    caps[i] = static_cast<uint32_t>(cap);
  }
}

// --- CDLP's own pieces ------------------------------------------------------

// a null bitmap means every row is dirty
__device__ __forceinline__ bool row_is_dirty(
    const uint32_t* __restrict__ dirty, uint32_t v) {
  return !dirty || ((dirty[v >> 5] >> (v & 31)) & 1);
}

// Mode key: higher count wins, then the lower label. 0 is "no label seen".
__device__ __forceinline__ uint64_t mode_key(uint32_t cnt, uint32_t label) {
  return (static_cast<uint64_t>(cnt) << 32) | static_cast<uint32_t>(~label);
}
__device__ __forceinline__ uint32_t mode_label(uint64_t key) {
  return ~static_cast<uint32_t>(key);
}

__device__ __forceinline__ uint64_t wave_max(uint64_t key) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    uint64_t o = __shfl_down(static_cast<unsigned long long>(key), d, 64);
    if (o > key) key = o;
  }
  return key;  // lane 0 holds the maximum
}

// block argmax of mode keys; an empty row (no key) keeps `own`
__device__ __forceinline__ void cdlp_block_argmax(uint64_t key,
                                                  uint32_t* out,
                                                  uint32_t own) {
  __shared__ uint64_t s_wave[kBlock / kWave];
  key = wave_max(key);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t best = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w)
      if (s_wave[w] > best) best = s_wave[w];
    *out = best ? mode_label(best) : own;
  }
  __syncthreads();
}

// LDS open-addressing (label, count) table of the wave and mid tiers
__device__ __forceinline__ void lds_count_insert(uint32_t* s_lab,
                                                 uint32_t* s_cnt,
                                                 uint32_t mask, uint32_t l) {
  uint32_t idx = slot_hash(l) & mask;
  for (;;) {
    uint32_t old = atomicCAS(&s_lab[idx], kSlotEmpty, l);
    if (old == kSlotEmpty || old == l) {
      atomicAdd(&s_cnt[idx], 1u);
      return;
    }
    idx = (idx + 1) & mask;
  }
}

// this thread's best key over slots first, first + step, ... of the table
__device__ __forceinline__ uint64_t lds_table_mode(const uint32_t* s_lab,
                                                   const uint32_t* s_cnt,
                                                   uint32_t cap,
                                                   uint32_t first,
                                                   uint32_t step) {
  uint64_t key = 0;
  for (uint32_t k = first; k < cap; k += step) {
    uint32_t c = s_cnt[k];
    if (c) {
      uint64_t cand = mode_key(c, s_lab[k]);
      if (cand > key) key = cand;
    }
  }
  return key;
}

// In every tier a row of degree 0 keeps its own label.

// thread-per-row register mode for deg <= kTierTinyDeg (most power-law
// rows): a wave-per-row ballot on a deg-3 row idles 61 lanes
__global__ void cdlp_tiny_kernel(const uint64_t* __restrict__ off1,
                                 const uint32_t* __restrict__ dst1,
                                 const uint64_t* __restrict__ off2,
                                 const uint32_t* __restrict__ dst2,
                                 const uint32_t* __restrict__ lab,
                                 const uint32_t* __restrict__ rows,
                                 uint64_t nrows, uint32_t v_begin,
                                 const uint32_t* __restrict__ dirty,
                                 uint32_t* __restrict__ next) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint32_t r = rows[i];
    if (!row_is_dirty(dirty, v_begin + r)) continue;
    AdjRow<uint32_t> row = adj_row<uint32_t>(off1, off2, r, v_begin);
    if (row.deg == 0) {
      next[r] = lab[row.v];
      continue;
    }
    uint32_t l[kTierTinyDeg];
#pragma unroll
    for (uint32_t k = 0; k < kTierTinyDeg; ++k)
      if (k < row.deg) l[k] = lab[row.at(dst1, dst2, k)];
    uint32_t best_lab = kSlotEmpty, best_cnt = 0;
    for (uint32_t k = 0; k < row.deg; ++k) {
      bool first = true;
      for (uint32_t j = 0; j < k; ++j)
        if (l[j] == l[k]) first = false;
      if (!first) continue;
      uint32_t cnt = 1;
      for (uint32_t j = k + 1; j < row.deg; ++j)
        if (l[j] == l[k]) ++cnt;
      if (cnt > best_cnt || (cnt == best_cnt && l[k] < best_lab)) {
        best_cnt = cnt;
        best_lab = l[k];
      }
    }
    next[r] = best_lab;
  }
}

// wave-per-row ballot mode, deg <= kTierSmallDeg (one lane per arc)
__global__ void cdlp_small_kernel(const uint64_t* __restrict__ off1,
                                  const uint32_t* __restrict__ dst1,
                                  const uint64_t* __restrict__ off2,
                                  const uint32_t* __restrict__ dst2,
                                  const uint32_t* __restrict__ lab,
                                  const uint32_t* __restrict__ rows,
                                  uint64_t nrows, uint32_t v_begin,
                                  const uint32_t* __restrict__ dirty,
                                  uint32_t* __restrict__ next) {
  const uint32_t lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < nrows;
       i += wstride) {
    uint32_t r = rows[i];
    if (!row_is_dirty(dirty, v_begin + r)) continue;
    AdjRow<uint32_t> row = adj_row<uint32_t>(off1, off2, r, v_begin);
    if (row.deg == 0) {
      if (lane == 0) next[r] = lab[row.v];
      continue;
    }
    uint32_t mylab = kSlotEmpty;
    if (lane < row.deg) mylab = lab[row.at(dst1, dst2, lane)];
    unsigned long long remaining = __ballot(lane < row.deg);
    uint32_t best_cnt = 0, best_lab = kSlotEmpty;
    while (remaining) {
      int L = __ffsll(remaining) - 1;
      uint32_t lab0 = __shfl(mylab, L, 64);
      unsigned long long m = __ballot(mylab == lab0) & remaining;
      remaining &= ~m;
      uint32_t cnt = __popcll(m);
      if (cnt > best_cnt || (cnt == best_cnt && lab0 < best_lab)) {
        best_cnt = cnt;
        best_lab = lab0;
      }
    }
    if (lane == 0) next[r] = best_lab;
  }
}

// 4-rows-per-block wave hash for kTierSmallDeg < deg <= kTierWaveDeg: a
// block-per-row table on a deg-100 row leaves 3 of 4 waves idle; here each
// wave owns a 1024-slot LDS region and the group loop is uniform so plain
// __syncthreads stages the clear/insert/reduce phases.
__global__ void cdlp_wave_kernel(const uint64_t* __restrict__ off1,
                                 const uint32_t* __restrict__ dst1,
                                 const uint64_t* __restrict__ off2,
                                 const uint32_t* __restrict__ dst2,
                                 const uint32_t* __restrict__ lab,
                                 const uint32_t* __restrict__ rows,
                                 uint64_t nrows, uint32_t v_begin,
                                 const uint32_t* __restrict__ dirty,
                                 uint32_t* __restrict__ next) {
  __shared__ uint32_t s_lab[4][kTierWaveSlots];
  __shared__ uint32_t s_cnt[4][kTierWaveSlots];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  uint64_t groups = (nrows + 3) / 4;
  for (uint64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    uint64_t i = grp * 4 + wid;
    bool have = i < nrows;
    uint32_t r = have ? rows[i] : 0;
    if (have && !row_is_dirty(dirty, v_begin + r)) have = false;
    AdjRow<uint32_t> row{};
    uint32_t cap = 64;
    if (have) {
      row = adj_row<uint32_t>(off1, off2, r, v_begin);
      cap = lds_table_cap(row.deg, kTierWaveSlots);
      for (uint32_t k = lane; k < cap; k += kWave) {
        s_lab[wid][k] = kSlotEmpty;
        s_cnt[wid][k] = 0;
      }
    }
    __syncthreads();
    if (have)
      for (uint32_t k = lane; k < row.deg; k += kWave)
        lds_count_insert(s_lab[wid], s_cnt[wid], cap - 1,
                         lab[row.at(dst1, dst2, k)]);
    __syncthreads();
    if (have) {
      uint64_t key =
          wave_max(lds_table_mode(s_lab[wid], s_cnt[wid], cap, lane, kWave));
      // no key: the row is empty (a row with arcs always counts a label)
      if (lane == 0) next[r] = key ? mode_label(key) : lab[row.v];
    }
    __syncthreads();
  }
}

// block-per-row LDS hash, kTierWaveDeg < deg <= kTierMidDeg
__global__ void cdlp_mid_kernel(const uint64_t* __restrict__ off1,
                                const uint32_t* __restrict__ dst1,
                                const uint64_t* __restrict__ off2,
                                const uint32_t* __restrict__ dst2,
                                const uint32_t* __restrict__ lab,
                                const uint32_t* __restrict__ rows,
                                uint64_t nrows, uint32_t v_begin,
                                const uint32_t* __restrict__ dirty,
                                uint32_t* __restrict__ next) {
  __shared__ uint32_t s_lab[kTierMidSlots];
  __shared__ uint32_t s_cnt[kTierMidSlots];
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    if (!row_is_dirty(dirty, v_begin + r)) continue;
    AdjRow<uint32_t> row = adj_row<uint32_t>(off1, off2, r, v_begin);
    const uint32_t cap = lds_table_cap(row.deg, kTierMidSlots);
    for (uint32_t k = threadIdx.x; k < cap; k += blockDim.x) {
      s_lab[k] = kSlotEmpty;
      s_cnt[k] = 0;
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < row.deg; k += blockDim.x)
      lds_count_insert(s_lab, s_cnt, cap - 1, lab[row.at(dst1, dst2, k)]);
    __syncthreads();
    cdlp_block_argmax(
        lds_table_mode(s_lab, s_cnt, cap, threadIdx.x, blockDim.x), &next[r],
        lab[row.v]);
  }
}

// Block-per-row global hash for rows past kTierMidDeg. Row i owns slots
// tbl_off[i] .. tbl_off[i + 1] of the pool. A slot is one u64: the high 32
// bits hold the label, the low 32 hold epoch:8 | count:24. A slot whose
// epoch is not this launch's reads as empty, so the pool is never cleared
// between iterations (the host re-zeroes it when the 8-bit epoch wraps;
// epoch 0 is the zeroed state and is never launched). The count saturates
// at 2^24 - 1.
__global__ void cdlp_large_kernel(const uint64_t* __restrict__ off1,
                                  const uint32_t* __restrict__ dst1,
                                  const uint64_t* __restrict__ off2,
                                  const uint32_t* __restrict__ dst2,
                                  const uint32_t* __restrict__ lab,
                                  const uint32_t* __restrict__ rows,
                                  uint64_t nrows,
                                  const uint64_t* __restrict__ tbl_off,
                                  unsigned long long* __restrict__ tbl,
                                  uint32_t epoch, uint32_t v_begin,
                                  const uint32_t* __restrict__ dirty,
                                  uint32_t* __restrict__ next) {
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    if (!row_is_dirty(dirty, v_begin + r)) continue;
    AdjRow<uint64_t> row = adj_row<uint64_t>(off1, off2, r, v_begin);
    uint64_t tb = tbl_off[i];
    const uint64_t cap = tbl_off[i + 1] - tb;
    const uint64_t mask = cap - 1;
    unsigned long long* t = tbl + tb;
    const uint32_t etag = epoch << 24;
    for (uint64_t k = threadIdx.x; k < row.deg; k += blockDim.x) {
      uint32_t l = lab[row.at(dst1, dst2, k)];
      uint64_t idx = slot_hash(l) & mask;
      for (;;) {
        unsigned long long cur = t[idx];
        uint32_t cur_lab = static_cast<uint32_t>(cur >> 32);
        uint32_t cur_lo = static_cast<uint32_t>(cur);
        bool stale = (cur_lo >> 24) != epoch;
        if (stale) {
          // try to claim the slot for this epoch with count 1
          unsigned long long want =
              (static_cast<unsigned long long>(l) << 32) | (etag | 1u);
          unsigned long long old = atomicCAS(&t[idx], cur, want);
          if (old == cur) break;      // claimed
          cur = old;                  // somebody else raced; re-inspect
          cur_lab = static_cast<uint32_t>(cur >> 32);
          cur_lo = static_cast<uint32_t>(cur);
          if ((cur_lo >> 24) != epoch) continue;  // still stale: retry slot
        }
        if (cur_lab == l) {
          if ((cur_lo & 0xFFFFFF) != 0xFFFFFF) atomicAdd(&t[idx], 1ull);
          break;
        }
        idx = (idx + 1) & mask;
      }
    }
    __syncthreads();
    uint64_t key = 0;
    for (uint64_t k = threadIdx.x; k < cap; k += blockDim.x) {
      unsigned long long cur = t[k];
      uint32_t lo = static_cast<uint32_t>(cur);
      if ((lo >> 24) == epoch && (lo & 0xFFFFFF)) {
        uint64_t cand =
            mode_key(lo & 0xFFFFFF, static_cast<uint32_t>(cur >> 32));
        if (cand > key) key = cand;
      }
    }
    cdlp_block_argmax(key, &next[r], lab[row.v]);
  }
}

__global__ void cdlp_commit_kernel(const uint32_t* __restrict__ next,
                                   uint32_t owned, uint32_t v_begin,
                                   const uint32_t* __restrict__ dirty,
                                   uint32_t* __restrict__ lab,
                                   DevBitmap changed,
                                   unsigned long long* __restrict__ nch) {
  __shared__ unsigned long long s_nch;
  if (threadIdx.x == 0) s_nch = 0;
  __syncthreads();
  unsigned long long my = 0;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride) {
    uint32_t v = v_begin + r;
    if (!row_is_dirty(dirty, v)) continue;
    uint32_t nv = next[r];
    if (nv != lab[v]) {
      lab[v] = nv;
      changed.set_once(r);
      ++my;
    }
  }
  if (my) atomicAdd(&s_nch, my);
  __syncthreads();
  if (threadIdx.x == 0 && s_nch) atomicAdd(nch, s_nch);
}

// mark rows whose label multiset can have changed: every neighbor of a
// changed vertex (undirected: out-CSR covers it; directed: out + in)
struct CdlpMarkOp {
  DevBitmap dirty;
  __device__ __forceinline__ void operator()(uint32_t v, uint32_t) const {
    dirty.set_once(v);
  }
};

struct CdlpDirtyOp {
  DevBitmap dirty;  // global-vid bitmap
  uint32_t v_begin, v_end;
  bool multi;
  DevHalo halo;
  __device__ __forceinline__ void operator()(uint32_t, uint32_t d,
                                             float) const {
    if (d >= v_begin && d < v_end) {
      dirty.set_once(d);
    } else if (multi) {
      halo.add(d);
    } else {
      dirty.set_once(d);
    }
  }
};

// Owned rows tiered by combined (off1 [+ off2]) degree, and the layout of
// the global table pool the large tier hashes into: large row i owns slots
// heavy_off[i] .. heavy_off[i + 1] of heavy_total. The pool itself is the
// user's (CDLP: epoch-tagged u64 slots, LCC: u32 labels). Built once per run;
// syncs s for the tier counts and, with large rows, for the pool size.
struct RowTiers {
  DeviceBuffer<uint32_t> tiny, small, wave, mid, large;
  uint64_t n_tiny = 0, n_small = 0, n_wave = 0, n_mid = 0, n_large = 0;
  DeviceBuffer<uint64_t> heavy_off;
  uint64_t heavy_total = 0;
};

static RowTiers build_row_tiers(const uint64_t* off1, const uint64_t* off2,
                                uint32_t owned, bool tiny, hipStream_t s,
                                ScanTemp& scan) {
  RowTiers t;
  auto n = partition_rows(
      CombinedDegTiers{off1, off2, tiny}, owned,
      {tiny ? &t.tiny : nullptr, &t.small, &t.wave, &t.mid, &t.large}, s);
  t.n_tiny = n[0], t.n_small = n[1], t.n_wave = n[2], t.n_mid = n[3],
  t.n_large = n[4];
  if (t.n_large) {
    DeviceBuffer<uint32_t> caps(t.n_large);
    t.heavy_off.resize(t.n_large + 1);
    heavy_cap_kernel<<<grid_for(t.n_large), kBlock, 0, s>>>(
        off1, off2, t.large.data(), t.n_large, caps.data());
    t.heavy_total =
        exclusive_scan(caps.data(), t.heavy_off.data(), t.n_large, s, scan);
  }
  return t;
}

// iteration `it` of the label mode over all five tiers into `next`
static void launch_cdlp_tiers(RowTiers& t, const uint64_t* o1,
                              const uint32_t* d1, const uint64_t* o2,
                              const uint32_t* d2, const uint32_t* lab,
                              DeviceBuffer<unsigned long long>& heavy_tbl,
                              int it, uint32_t v_begin, const uint32_t* dirty,
                              uint32_t* next, hipStream_t s) {
  if (t.n_tiny)
    cdlp_tiny_kernel<<<grid_for(t.n_tiny), kBlock, 0, s>>>(
        o1, d1, o2, d2, lab, t.tiny.data(), t.n_tiny, v_begin, dirty, next);
  if (t.n_small)
    cdlp_small_kernel<<<grid_for(t.n_small * kWave), kBlock, 0, s>>>(
        o1, d1, o2, d2, lab, t.small.data(), t.n_small, v_begin, dirty, next);
  if (t.n_wave)
    cdlp_wave_kernel<<<grid_for(((t.n_wave + 3) / 4) * kBlock), kBlock, 0,
                       s>>>(o1, d1, o2, d2, lab, t.wave.data(), t.n_wave,
                            v_begin, dirty, next);
  if (t.n_mid)
    cdlp_mid_kernel<<<std::min<int>(t.n_mid, kMaxGrid), kBlock, 0, s>>>(
        o1, d1, o2, d2, lab, t.mid.data(), t.n_mid, v_begin, dirty, next);
  if (t.n_large) {
    // the epoch tag is 8-bit and 0 is the zeroed state: re-zero on wrap
    if (it > 0 && it % 254 == 0) heavy_tbl.zero(s);
    cdlp_large_kernel<<<std::min<int>(t.n_large, kMaxGrid), kBlock, 0, s>>>(
        o1, d1, o2, d2, lab, t.large.data(), t.n_large, t.heavy_off.data(),
        heavy_tbl.data(), static_cast<uint32_t>((it % 254) + 1), v_begin,
        dirty, next);
  }
}

GpuRunResult GpuContext::cdlp(DeviceGraph& g, int iters, bool fetch) {
  RangeMarker _mk("grapehip::cdlp");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  bool multi = world_ > 1;
  if (g.directed && !g.has_in)
    throw std::runtime_error(
        "GPU CDLP on a directed graph needs the in-CSR "
        "(load with build_in_csr=True)");

  const uint64_t* off1 = g.oe_off.data();
  const uint32_t* dst1 = g.oe_dst.data();
  const uint64_t* off2 = g.directed ? g.ie_off.data() : nullptr;
  const uint32_t* dst2 = g.directed ? g.ie_dst.data() : nullptr;

  // tier the rows once (degrees don't change across iterations); the
  // heavy-row pool is zeroed once (epoch 0 == the virgin state)
  RowTiers tiers = build_row_tiers(off1, off2, owned, true, s, I.scan);
  DeviceBuffer<unsigned long long> heavy_tbl(tiers.heavy_total);
  heavy_tbl.zero(s);

  DeviceBuffer<uint32_t> lab(nv_pad);
  DeviceBuffer<uint32_t> next(owned ? owned : 1);
  // delta-convergence machinery: only rows with a changed neighborhood
  // recompute their mode (exact: an unchanged multiset reproduces the
  // same mode); fixpoint exits early
  size_t dirty_words = (static_cast<size_t>(nv_pad) + 31) / 32 + 1;
  DeviceBuffer<uint32_t> dirty(dirty_words);
  DeviceBuffer<uint32_t> changed_bm((owned + 31) / 32 + 1);
  DeviceBuffer<uint32_t> changed_q(owned ? owned : 1);
  DeviceBuffer<unsigned long long> d_nch(1);
  uint64_t halo_cap = nv_pad / (world_ ? world_ : 1);
  DevGraphView view = make_view(g, rank_, world_);
  const DevHalo halo =
      halo_reserve(I, world_, halo_cap, view.slice, dirty_words);
  if (multi) halo_reset(I, s);
  DevGraphView view_in = view;
  if (g.directed) {
    view_in.oe_off = g.ie_off.data();
    view_in.oe_dst = g.ie_dst.data();
    view_in.oe_w = nullptr;
  }
  if (multi) ensure_mirrors(I, comm_, g, rank_, world_, s);

  RunBracket br(I, comm_);

  // label space must compare in OID order (reference tie-break): dense
  // renumber uses the sorted-oid table, hub renumber the inverse perm
  const uint32_t* lab0 = g.oid_order.size()
                             ? g.oid_order.data()
                             : (g.permuted ? g.inv.data() : nullptr);
  if (lab0)
    HIP_CHECK(hipMemcpyAsync(lab.data(), lab0,
                             static_cast<size_t>(nv_pad) * 4,
                             hipMemcpyDeviceToDevice, s));
  else
    iota_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(lab.data(), 0, nv_pad);
  changed_bm.zero(s);
  int rounds = 0;
  bool use_dirty = false;  // iteration 0 recomputes everything
  for (int it = 0; it < iters; ++it) {
    const uint32_t* dw = use_dirty ? dirty.data() : nullptr;
    launch_cdlp_tiers(tiers, off1, dst1, off2, dst2, lab.data(), heavy_tbl,
                      it, g.v_begin, dw, next.data(), s);
    d_nch.zero(s);
    if (owned)
      cdlp_commit_kernel<<<grid_for(owned), kBlock, 0, s>>>(
          next.data(), owned, g.v_begin, dw, lab.data(),
          DevBitmap{changed_bm.data()}, d_nch.data());
    ++rounds;
    unsigned long long nch = 0;
    HIP_CHECK(hipMemcpyAsync(&nch, d_nch.data(), 8, hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t g_nch = multi ? comm_->allreduce_sum(nch) : nch;
    if (g_nch == 0) break;  // fixpoint: nothing changed, nothing to sync
    if (multi) {
      // refresh referenced remote labels point-to-point (per-link volume
      // scales with boundary size, not V·world); once churn decays,
      // ship only the CHANGED labels as (id, value) pairs
      uint64_t g_owned_now =
          comm_->allreduce_sum(static_cast<uint64_t>(owned));
      if (g_nch * 8 < g_owned_now) {
        mirror_sync_changed(I, comm_, g, lab.data(), changed_bm.data(),
                            rank_, world_, s);
      } else {
        mirror_sync_begin(I, g, lab.data(), s);
        mirror_sync_end(I, g, lab.data(), s);
      }
    }
    if (it + 1 == iters) break;
    // adaptive: building the dirty set costs an edge expansion over the
    // changed rows — only worth it once changes are sparse (converging
    // graphs); with heavy churn (early rounds, RMAT oscillation) a full
    // recompute is cheaper than sweep + marking
    uint64_t g_owned =
        multi ? comm_->allreduce_sum(static_cast<uint64_t>(owned))
              : owned;
    use_dirty = g_nch < g_owned / 8;
    if (!use_dirty) {
      changed_bm.zero(s);
      continue;
    }
    // rebuild the dirty set from this round's changed rows
    dirty.zero(s);
    uint64_t qn = compact_frontier(I, changed_bm.data(), owned, g.v_begin,
                                   changed_q.data(), s);
    if (qn) {
      CdlpDirtyOp op{DevBitmap{dirty.data()}, g.v_begin, g.v_end, multi,
                     halo};
      expand_frontier(I, view, changed_q.data(),
                      static_cast<uint32_t>(qn), op, s);
      if (g.directed)
        expand_frontier(I, view_in, changed_q.data(),
                        static_cast<uint32_t>(qn), op, s);
    }
    if (multi)
      halo_round<uint32_t>(I, comm_, rank_, world_, lab.data(), halo_cap,
                           CdlpMarkOp{DevBitmap{dirty.data()}}, s);
  }
  GpuRunResult res = br.finish(
      rounds,
      static_cast<uint64_t>(iters) * g.total_edges * (g.directed ? 2 : 1));
  if (fetch) {
    std::vector<uint32_t> l32(owned);
    HIP_CHECK(hipMemcpyAsync(l32.data(), lab.data() + g.v_begin, owned * 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    res.i64.assign(l32.begin(), l32.end());
  }
  return res;
}
// ---------------------------------------------------------------------------
// LCC (local clustering coefficient; reference examples/analytical_apps/
// cuda/lcc/lcc.h). LDBC semantics (matches the CPU app in apps/lcc.hpp):
//   D(v) = |distinct in∪out neighbors, excl. self|
//   lcc(v) = 2·tri(v) / (D(v)·(D(v)−1))
// MI355X pipeline (no CUB segmented radix — hash dedup + LDS bitonic):
//   1. D(v) per owned row via degree-tiered hash distinct-count
//      (wave-ballot / LDS hash / global hash — same tiers as CDLP)
//   2. allgather D over xGMI (replicated u32 array)
//   3. oriented adjacency O(v) = {u ∈ N(v) : (D(u),u) > (D(v),v)}, deduped
//      during the same hash pass; each edge u—v survives in exactly one
//      direction, so Σ|O| = E_simple/… and every triangle is found once
//   4. per-row ascending sort of O(v): LDS bitonic ≤4096, global scratch
//      bitonic for heavier rows (reference uses CUB SegmentedRadixSort,
//      cuda/utils/cuda_utils.h:194-290)
//   5. ragged allgather of the oriented CSR (per-rank region broadcast)
//   6. wave-per-row intersection count: for each oriented edge (u,v),
//      merge-intersect O(u)∩O(v);每 hit credits u, v, w (atomicAdd u64)
//   7. allreduce-sum T, finalize lcc = 2T/(D(D−1))
// ---------------------------------------------------------------------------

// orientation: keep u in O(v) iff (D[u],u) > (D[v],v)
__device__ __forceinline__ bool lcc_keep(uint32_t du, uint32_t u, uint32_t dv,
                                         uint32_t v) {
  return du > dv || (du == dv && u > v);
}

// --- tiered dedup pass (passes 1 and 3 above) -----------------------------
// Every tier walks a row of the combined (off1 [+ off2]) adjacency and sees
// each u != v once; what happens on that first occurrence is the sink's:
//   LccCountSink  counts them and writes D[v]
//   LccEmitSink   appends them (orientation-filtered when `filter`) to the
//                 row's capacity-layout slot in oadj and writes ocnt[r]

// open-addressing insert into a pow2 table (LDS: u32 mask, global: u64
// mask); true iff u was not there yet
template <typename Mask>
__device__ __forceinline__ bool insert_once(uint32_t* table, Mask mask,
                                            uint32_t u) {
  Mask idx = slot_hash(u) & mask;
  for (;;) {
    uint32_t old = atomicCAS(&table[idx], kSlotEmpty, u);
    if (old == kSlotEmpty) return true;
    if (old == u) return false;
    idx = (idx + 1) & mask;
  }
}

// small tier (deg <= 64, one lane per arc): bit L set iff lane L holds the
// first occurrence of its value among the active lanes
__device__ __forceinline__ unsigned long long lcc_first_mask(uint32_t u,
                                                             bool active) {
  unsigned long long remaining = __ballot(active);
  unsigned long long first_mask = 0;
  while (remaining) {
    int L = __ffsll(remaining) - 1;
    uint32_t u0 = __shfl(u, L, 64);
    first_mask |= (1ull << L);
    remaining &= ~__ballot(active && u == u0);
  }
  return first_mask;
}

// A sink supplies: Row open(r, v) once the row's counter n is zeroed;
// first(row, u, v, &n) on a first occurrence (n is the tier's LDS counter);
// close(r, v, n) by one thread when the row is done; and small(...) for the
// table-less tier, called by the whole wave with the first-occurrence mask.
struct LccCountSink {
  uint32_t* D;
  struct Row {};
  __device__ __forceinline__ Row open(uint32_t, uint32_t) const { return {}; }
  __device__ __forceinline__ void first(const Row&, uint32_t, uint32_t,
                                        uint32_t* n) const {
    atomicAdd(n, 1u);
  }
  __device__ __forceinline__ void close(uint32_t, uint32_t v,
                                        uint32_t n) const {
    D[v] = n;
  }
  __device__ __forceinline__ void small(uint32_t, uint32_t v, int lane,
                                        uint32_t, bool,
                                        unsigned long long first_mask) const {
    if (lane == 0) D[v] = __popcll(first_mask);
  }
};

struct LccEmitSink {
  const uint32_t* D;
  const uint64_t* ooff;
  uint32_t* oadj;
  uint32_t* ocnt;
  bool filter;
  struct Row {
    uint32_t dv;
    uint64_t base;
  };
  __device__ __forceinline__ Row open(uint32_t r, uint32_t v) const {
    return {D[v], ooff[r]};
  }
  __device__ __forceinline__ bool wants(const Row& row, uint32_t u,
                                        uint32_t v) const {
    return !filter || lcc_keep(D[u], u, row.dv, v);
  }
  __device__ __forceinline__ void first(const Row& row, uint32_t u,
                                        uint32_t v, uint32_t* n) const {
    if (wants(row, u, v)) oadj[row.base + atomicAdd(n, 1u)] = u;
  }
  __device__ __forceinline__ void close(uint32_t r, uint32_t,
                                        uint32_t n) const {
    ocnt[r] = n;
  }
  __device__ __forceinline__ void small(uint32_t r, uint32_t v, int lane,
                                        uint32_t u, bool active,
                                        unsigned long long first_mask) const {
    Row row = open(r, v);
    bool keep = active && ((first_mask >> lane) & 1) && wants(row, u, v);
    unsigned long long keep_mask = __ballot(keep);
    uint32_t pos = __popcll(keep_mask & ((1ull << lane) - 1));
    if (keep) oadj[row.base + pos] = u;
    if (lane == 0) ocnt[r] = __popcll(keep_mask);
  }
};

template <typename Sink>
__global__ void lcc_dedup_small_kernel(
    const uint64_t* __restrict__ off1, const uint32_t* __restrict__ dst1,
    const uint64_t* __restrict__ off2, const uint32_t* __restrict__ dst2,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    Sink sink) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < nrows;
       i += wstride) {
    uint32_t r = rows[i];
    AdjRow<uint32_t> row = adj_row<uint32_t>(off1, off2, r, v_begin);
    uint32_t u = kSlotEmpty;
    if (lane < static_cast<int>(row.deg))
      u = row.at(dst1, dst2, static_cast<uint32_t>(lane));
    bool active = lane < static_cast<int>(row.deg) && u != row.v;
    sink.small(r, row.v, lane, u, active, lcc_first_mask(u, active));
  }
}

// 4 rows per block for 64 < deg <= kTierWaveDeg (a block-per-row hash on a
// deg-100 row idles 3 of 4 waves; same uniform-barrier staging as
// cdlp_wave_kernel)
template <typename Sink>
__global__ void lcc_dedup_wave_kernel(
    const uint64_t* __restrict__ off1, const uint32_t* __restrict__ dst1,
    const uint64_t* __restrict__ off2, const uint32_t* __restrict__ dst2,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    Sink sink) {
  __shared__ uint32_t s_lab[4][kTierWaveSlots];
  __shared__ uint32_t s_n[4];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  uint64_t groups = (nrows + 3) / 4;
  for (uint64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    uint64_t i = grp * 4 + wid;
    const bool have = i < nrows;
    uint32_t r = have ? rows[i] : 0;
    AdjRow<uint32_t> row{};
    uint32_t mask = 63;
    if (have) {
      row = adj_row<uint32_t>(off1, off2, r, v_begin);
      uint32_t cap = lds_table_cap(row.deg, kTierWaveSlots);
      mask = cap - 1;
      for (uint32_t k = lane; k < cap; k += kWave)
        s_lab[wid][k] = kSlotEmpty;
      if (lane == 0) s_n[wid] = 0;
    }
    __syncthreads();
    if (have) {
      auto st = sink.open(r, row.v);
      for (uint32_t k = lane; k < row.deg; k += kWave) {
        uint32_t u = row.at(dst1, dst2, k);
        if (u == row.v) continue;
        if (insert_once(s_lab[wid], mask, u))
          sink.first(st, u, row.v, &s_n[wid]);
      }
    }
    __syncthreads();
    if (have && lane == 0) sink.close(r, row.v, s_n[wid]);
    __syncthreads();
  }
}

template <typename Sink>
__global__ void lcc_dedup_mid_kernel(
    const uint64_t* __restrict__ off1, const uint32_t* __restrict__ dst1,
    const uint64_t* __restrict__ off2, const uint32_t* __restrict__ dst2,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    Sink sink) {
  __shared__ uint32_t s_lab[kTierMidSlots];
  __shared__ uint32_t s_n;
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    AdjRow<uint32_t> row = adj_row<uint32_t>(off1, off2, r, v_begin);
    const uint32_t cap = lds_table_cap(row.deg, kTierMidSlots);
    const uint32_t mask = cap - 1;
    for (uint32_t k = threadIdx.x; k < cap; k += blockDim.x)
      s_lab[k] = kSlotEmpty;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    auto st = sink.open(r, row.v);
    for (uint32_t k = threadIdx.x; k < row.deg; k += blockDim.x) {
      uint32_t u = row.at(dst1, dst2, k);
      if (u == row.v) continue;
      if (insert_once(s_lab, mask, u)) sink.first(st, u, row.v, &s_n);
    }
    __syncthreads();
    if (threadIdx.x == 0) sink.close(r, row.v, s_n);
    __syncthreads();
  }
}

// rows past kTierMidDeg: row i hashes into its slice of the global table
// pool (tbl_off[i] .. tbl_off[i + 1]), which the host clears before launch
template <typename Sink>
__global__ void lcc_dedup_large_kernel(
    const uint64_t* __restrict__ off1, const uint32_t* __restrict__ dst1,
    const uint64_t* __restrict__ off2, const uint32_t* __restrict__ dst2,
    const uint32_t* __restrict__ rows, uint64_t nrows,
    const uint64_t* __restrict__ tbl_off, uint32_t* __restrict__ tbl_lab,
    uint32_t v_begin, Sink sink) {
  __shared__ uint32_t s_n;
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    AdjRow<uint64_t> row = adj_row<uint64_t>(off1, off2, r, v_begin);
    uint64_t tb = tbl_off[i];
    const uint64_t mask = (tbl_off[i + 1] - tb) - 1;
    uint32_t* tl = tbl_lab + tb;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    auto st = sink.open(r, row.v);
    for (uint64_t k = threadIdx.x; k < row.deg; k += blockDim.x) {
      uint32_t u = row.at(dst1, dst2, k);
      if (u == row.v) continue;
      if (insert_once(tl, mask, u)) sink.first(st, u, row.v, &s_n);
    }
    __syncthreads();
    if (threadIdx.x == 0) sink.close(r, row.v, s_n);
    __syncthreads();
  }
}

// compact capacity-layout rows into the tight global CSR region
__global__ void lcc_compact_kernel(const uint64_t* __restrict__ ooff,
                                   const uint32_t* __restrict__ ocnt,
                                   const uint32_t* __restrict__ oadj,
                                   const uint64_t* __restrict__ goff,
                                   uint32_t owned, uint32_t v_begin,
                                   uint32_t* __restrict__ gdst) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < owned;
       i += wstride) {
    uint32_t n = ocnt[i];
    uint64_t src = ooff[i];
    uint64_t dstb = goff[v_begin + i];
    for (uint32_t k = lane; k < n; k += kWave) gdst[dstb + k] = oadj[src + k];
  }
}

// Triangle counting via per-vertex hash sets of oriented neighbors.
// v2 history: per-lane serial merge rescanned O(u) per edge (quadratic in
// hub rows); binary search made it WORSE (log n random reads beat by the
// merge's streaming locality — 2.3s -> 3.7s at 40M). Hash probing is O(1)
// random reads per element: enumerate the smaller list, probe the larger
// list's open-addressing set. Tables are built once over the exchanged
// oriented CSR (capacity 2x, pow2), ~8 bytes per oriented edge of HBM.
__global__ void lcc_hashcap_kernel(const uint64_t* __restrict__ goff,
                                   uint32_t nv, uint32_t* __restrict__ caps) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    uint64_t n = goff[v + 1] - goff[v];
    uint64_t cap = 1;  // empty rows are never probed
    if (n) {
      cap = 4;
      while (cap < 2 * n) cap <<= 1;
    }
    caps[v] = static_cast<uint32_t>(cap);
  }
}

__global__ void lcc_hashfill_kernel(const uint64_t* __restrict__ goff,
                                    const uint32_t* __restrict__ gdst,
                                    const uint64_t* __restrict__ hoff,
                                    uint32_t nv,
                                    uint32_t* __restrict__ htab) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.x) * wpb + wid; v < nv;
       v += wstride) {
    uint64_t b = goff[v];
    uint32_t n = static_cast<uint32_t>(goff[v + 1] - b);
    if (n == 0) continue;
    uint64_t hb = hoff[v];
    const uint64_t mask = (hoff[v + 1] - hb) - 1;
    uint32_t* t = htab + hb;
    for (uint32_t k = lane; k < n; k += kWave)
      (void)insert_once(t, mask, gdst[b + k]);
  }
}

__device__ __forceinline__ bool lcc_probe(const uint32_t* __restrict__ t,
                                          uint64_t mask, uint32_t key) {
  uint64_t idx = slot_hash(key) & mask;
  for (;;) {
    uint32_t x = t[idx];
    if (x == key) return true;
    if (x == kSlotEmpty) return false;
    idx = (idx + 1) & mask;
  }
}

// Light-edge pass, two tiers by oriented row size:
//   wee rows (un <= 32): wave-per-row, lanes probe global hash sets
//   staged rows: block-per-row; the row's hash set is staged into LDS once
//   and every thread's probes hit LDS (the global-probe version spent its
//   time on scattered 4B HBM reads; witness atomics measured ~5%)
constexpr uint32_t kLccWeeRows = 768;  // swept 32/256/768/2048: 3206/2750/2607/2713 ms at datagen-9_0
constexpr uint32_t kLccStageSlots = 8192;  // 32 KB LDS

__global__ void lcc_tri_wee_kernel(const uint64_t* __restrict__ goff,
                                   const uint32_t* __restrict__ gdst,
                                   const uint64_t* __restrict__ hoff,
                                   const uint32_t* __restrict__ htab,
                                   const uint32_t* __restrict__ rows,
                                   uint64_t nrows, uint32_t v_begin,
                                   unsigned long long* __restrict__ T,
                                   uint32_t heavy_thresh,
                                   unsigned long long* __restrict__ heavy_q,
                                   unsigned long long* __restrict__ heavy_n,
                                   bool skip_witness) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < nrows;
       i += wstride) {
    uint32_t u = v_begin + rows[i];
    uint64_t ub = goff[u];
    uint32_t un = static_cast<uint32_t>(goff[u + 1] - ub);
    unsigned long long my_u = 0;
    for (uint32_t k = lane; k < un; k += kWave) {
      uint32_t v = gdst[ub + k];
      uint64_t vb = goff[v];
      uint32_t vn = static_cast<uint32_t>(goff[v + 1] - vb);
      if (vn == 0) continue;
      uint32_t mn = vn < un ? vn : un;
      if (mn > heavy_thresh) {
        heavy_q[atomicAdd(heavy_n, 1ull)] =
            (static_cast<unsigned long long>(u) << 32) | v;
        continue;
      }
      uint64_t eb, hb;
      uint32_t en;
      uint64_t mask;
      if (vn < un) {
        eb = vb;
        en = vn;
        hb = hoff[u];
        mask = (hoff[u + 1] - hb) - 1;
      } else {
        eb = ub;
        en = un;
        hb = hoff[v];
        mask = (hoff[v + 1] - hb) - 1;
      }
      const uint32_t* t = htab + hb;
      unsigned long long hits = 0;
      // 4 interleaved probe chains (see the heavy kernel): the serial
      // dependent probe left the wave parked on latency
      for (uint32_t e0 = 0; e0 < en; e0 += 4) {
        uint32_t key[4];
        uint64_t idx[4];
        bool live[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          live[j] = e0 + j < en;
          key[j] = live[j] ? gdst[eb + e0 + j] : 0;
          idx[j] = slot_hash(key[j]) & mask;
        }
        for (;;) {
          uint32_t x[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (live[j]) x[j] = t[idx[j]];
          bool any = false;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!live[j]) continue;
            if (x[j] == key[j]) {
              ++hits;
              if (!skip_witness) atomicAdd(&T[key[j]], 1ull);
              live[j] = false;
            } else if (x[j] == kSlotEmpty) {
              live[j] = false;
            } else {
              idx[j] = (idx[j] + 1) & mask;
              any = true;
            }
          }
          if (!any) break;
        }
      }
      if (hits) {
        my_u += hits;
        atomicAdd(&T[v], hits);
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
      my_u += __shfl_down(my_u, d, 64);
    if (lane == 0 && my_u) atomicAdd(&T[u], my_u);
  }
}

__device__ __forceinline__ bool lcc_probe_lds(
    const uint32_t* __restrict__ t, uint32_t mask, uint32_t key) {
  uint32_t idx = slot_hash(key) & mask;
  for (;;) {
    uint32_t x = t[idx];
    if (x == key) return true;
    if (x == kSlotEmpty) return false;
    idx = (idx + 1) & mask;
  }
}

__global__ void lcc_tri_staged_kernel(
    const uint64_t* __restrict__ goff, const uint32_t* __restrict__ gdst,
    const uint64_t* __restrict__ hoff, const uint32_t* __restrict__ htab,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    unsigned long long* __restrict__ T, uint32_t heavy_thresh,
    unsigned long long* __restrict__ heavy_q,
    unsigned long long* __restrict__ heavy_n, bool skip_witness) {
  __shared__ uint32_t s_tab[kLccStageSlots];
  __shared__ unsigned long long s_hits;
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t u = v_begin + rows[i];
    uint64_t ub = goff[u];
    uint32_t un = static_cast<uint32_t>(goff[u + 1] - ub);
    uint64_t hb = hoff[u];
    uint32_t ucap = static_cast<uint32_t>(hoff[u + 1] - hb);
    const bool stage = ucap <= kLccStageSlots;
    if (stage)
      for (uint32_t k = threadIdx.x; k < ucap; k += blockDim.x)
        s_tab[k] = htab[hb + k];
    if (threadIdx.x == 0) s_hits = 0;
    __syncthreads();
    const uint32_t umask = ucap - 1;
    const uint32_t* ut = htab + hb;
    unsigned long long my_u = 0;
    for (uint32_t k = threadIdx.x; k < un; k += blockDim.x) {
      uint32_t v = gdst[ub + k];
      uint64_t vb = goff[v];
      uint32_t vn = static_cast<uint32_t>(goff[v + 1] - vb);
      if (vn == 0) continue;
      uint32_t mn = vn < un ? vn : un;
      if (mn > heavy_thresh) {
        heavy_q[atomicAdd(heavy_n, 1ull)] =
            (static_cast<unsigned long long>(u) << 32) | v;
        continue;
      }
      unsigned long long hits = 0;
      if (vn < un) {
        // enumerate O(v), probe u's set (LDS when staged)
        for (uint32_t e = 0; e < vn; ++e) {
          uint32_t w = gdst[vb + e];
          bool hit = stage ? lcc_probe_lds(s_tab, umask, w)
                           : lcc_probe(ut, umask, w);
          if (hit) {
            ++hits;
            if (!skip_witness) atomicAdd(&T[w], 1ull);
          }
        }
      } else {
        // enumerate O(u) (streamed, shared), probe v's global set
        uint64_t vhb = hoff[v];
        const uint64_t vmask = (hoff[v + 1] - vhb) - 1;
        const uint32_t* vt = htab + vhb;
        for (uint32_t e = 0; e < un; ++e) {
          uint32_t w = gdst[ub + e];
          if (lcc_probe(vt, vmask, w)) {
            ++hits;
            if (!skip_witness) atomicAdd(&T[w], 1ull);
          }
        }
      }
      if (hits) {
        my_u += hits;
        atomicAdd(&T[v], hits);
      }
    }
    if (my_u) atomicAdd(&s_hits, my_u);
    __syncthreads();
    if (threadIdx.x == 0 && s_hits) atomicAdd(&T[u], s_hits);
    __syncthreads();
  }
}

// the two light count tiers by global-CSR row length; rows shorter than
// min_n are skipped (1 undirected: empty rows; 2 directed: a lone neighbor
// closes no pair)
struct LccLenTiers {
  static constexpr int kLists = 2, kBins = 2;
  const uint64_t* __restrict__ goff;
  uint32_t v_begin, min_n;
  __device__ __forceinline__ int operator()(uint32_t r) const {
    uint64_t n = goff[v_begin + r + 1] - goff[v_begin + r];
    return n < min_n ? -1 : (n <= kLccWeeRows ? 0 : 1);
  }
};

// second pass: one wave per heavy edge; lanes stride the smaller list
__global__ void lcc_triangle_heavy_kernel(
    const uint64_t* __restrict__ goff, const uint32_t* __restrict__ gdst,
    const uint64_t* __restrict__ hoff, const uint32_t* __restrict__ htab,
    const unsigned long long* __restrict__ heavy_q, uint64_t heavy_n,
    unsigned long long* __restrict__ T) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid;
       i < heavy_n; i += wstride) {
    unsigned long long pk = heavy_q[i];
    uint32_t u = static_cast<uint32_t>(pk >> 32);
    uint32_t v = static_cast<uint32_t>(pk);
    uint64_t ub = goff[u];
    uint32_t un = static_cast<uint32_t>(goff[u + 1] - ub);
    uint64_t vb = goff[v];
    uint32_t vn = static_cast<uint32_t>(goff[v + 1] - vb);
    uint64_t eb, hb_big, hcap_end;
    uint32_t en;
    if (vn < un) {
      eb = vb;
      en = vn;
      hb_big = hoff[u];
      hcap_end = hoff[u + 1];
    } else {
      eb = ub;
      en = un;
      hb_big = hoff[v];
      hcap_end = hoff[v + 1];
    }
    const uint64_t mask = (hcap_end - hb_big) - 1;
    const uint32_t* t = htab + hb_big;
    unsigned long long hits = 0;
    // four probe state machines per lane: the single dependent probe chain
    // left waves 93% parked on memory latency (PMC r01); 4 outstanding
    // loads per lane quadruples the memory-level parallelism
    for (uint32_t e0 = lane; e0 < en; e0 += kWave * 4) {
      uint32_t key[4];
      uint64_t idx[4];
      bool live[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t e = e0 + j * kWave;
        live[j] = e < en;
        key[j] = live[j] ? gdst[eb + e] : 0;
        idx[j] = slot_hash(key[j]) & mask;
      }
      for (;;) {
        uint32_t x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (live[j]) x[j] = t[idx[j]];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!live[j]) continue;
          if (x[j] == key[j]) {
            ++hits;
            atomicAdd(&T[key[j]], 1ull);
            live[j] = false;
          } else if (x[j] == kSlotEmpty) {
            live[j] = false;
          } else {
            idx[j] = (idx[j] + 1) & mask;
            any = true;
          }
        }
        if (!any) break;
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
      hits += __shfl_down(hits, d, 64);
    if (lane == 0 && hits) {
      atomicAdd(&T[u], hits);
      atomicAdd(&T[v], hits);
    }
  }
}

// --- directed LCC (reference cuda/lcc/lcc_directed*.h semantics) ---------
// numerator(v) = sum over u in N(v) of |N(v) ∩ Nout(u)| computed directly
// (no orientation trick applies to the directed definition). Same light
// tiers as the undirected counter: wee rows wave-per-row with global
// probes; bigger rows block-per-row with U(v)'s hash set staged in LDS.
__global__ void lcc_dir_count_wee_kernel(
    const uint64_t* __restrict__ goffU, const uint32_t* __restrict__ gdstU,
    const uint64_t* __restrict__ hoffU, const uint32_t* __restrict__ htabU,
    const uint64_t* __restrict__ goffO, const uint32_t* __restrict__ gdstO,
    const uint64_t* __restrict__ hoffO, const uint32_t* __restrict__ htabO,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    unsigned long long* __restrict__ T, uint32_t heavy_thresh,
    unsigned long long* __restrict__ heavy_q,
    unsigned long long* __restrict__ heavy_n) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < nrows;
       i += wstride) {
    uint32_t v = v_begin + rows[i];
    uint64_t ub = goffU[v];
    uint32_t un = static_cast<uint32_t>(goffU[v + 1] - ub);
    unsigned long long my_v = 0;
    for (uint32_t k = lane; k < un; k += kWave) {
      uint32_t u = gdstU[ub + k];
      uint64_t ob = goffO[u];
      uint32_t on = static_cast<uint32_t>(goffO[u + 1] - ob);
      if (on == 0) continue;
      uint32_t mn = on < un ? on : un;
      if (mn > heavy_thresh) {
        heavy_q[atomicAdd(heavy_n, 1ull)] =
            (static_cast<unsigned long long>(v) << 32) | u;
        continue;
      }
      unsigned long long hits = 0;
      if (on <= un) {
        const uint64_t mask = (hoffU[v + 1] - hoffU[v]) - 1;
        const uint32_t* t = htabU + hoffU[v];
        for (uint32_t e = 0; e < on; ++e)
          if (lcc_probe(t, mask, gdstO[ob + e])) ++hits;
      } else {
        const uint64_t mask = (hoffO[u + 1] - hoffO[u]) - 1;
        const uint32_t* t = htabO + hoffO[u];
        for (uint32_t e = 0; e < un; ++e)
          if (lcc_probe(t, mask, gdstU[ub + e])) ++hits;
      }
      my_v += hits;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
      my_v += __shfl_down(my_v, d, 64);
    if (lane == 0 && my_v) atomicAdd(&T[v], my_v);
  }
}

__global__ void lcc_dir_count_staged_kernel(
    const uint64_t* __restrict__ goffU, const uint32_t* __restrict__ gdstU,
    const uint64_t* __restrict__ hoffU, const uint32_t* __restrict__ htabU,
    const uint64_t* __restrict__ goffO, const uint32_t* __restrict__ gdstO,
    const uint64_t* __restrict__ hoffO, const uint32_t* __restrict__ htabO,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    unsigned long long* __restrict__ T, uint32_t heavy_thresh,
    unsigned long long* __restrict__ heavy_q,
    unsigned long long* __restrict__ heavy_n) {
  __shared__ uint32_t s_tab[kLccStageSlots];
  __shared__ unsigned long long s_hits;
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t v = v_begin + rows[i];
    uint64_t ub = goffU[v];
    uint32_t un = static_cast<uint32_t>(goffU[v + 1] - ub);
    uint64_t hb = hoffU[v];
    uint32_t ucap = static_cast<uint32_t>(hoffU[v + 1] - hb);
    const bool stage = ucap <= kLccStageSlots;
    if (stage)
      for (uint32_t k = threadIdx.x; k < ucap; k += blockDim.x)
        s_tab[k] = htabU[hb + k];
    if (threadIdx.x == 0) s_hits = 0;
    __syncthreads();
    const uint32_t umask = ucap - 1;
    const uint32_t* ut = htabU + hb;
    unsigned long long my_v = 0;
    for (uint32_t k = threadIdx.x; k < un; k += blockDim.x) {
      uint32_t u = gdstU[ub + k];
      uint64_t ob = goffO[u];
      uint32_t on = static_cast<uint32_t>(goffO[u + 1] - ob);
      if (on == 0) continue;
      uint32_t mn = on < un ? on : un;
      if (mn > heavy_thresh) {
        heavy_q[atomicAdd(heavy_n, 1ull)] =
            (static_cast<unsigned long long>(v) << 32) | u;
        continue;
      }
      unsigned long long hits = 0;
      if (on <= un) {
        for (uint32_t e = 0; e < on; ++e) {
          uint32_t w = gdstO[ob + e];
          bool hit = stage ? lcc_probe_lds(s_tab, umask, w)
                           : lcc_probe(ut, umask, w);
          if (hit) ++hits;
        }
      } else {
        uint64_t ohb = hoffO[u];
        const uint64_t omask = (hoffO[u + 1] - ohb) - 1;
        const uint32_t* ot = htabO + ohb;
        for (uint32_t e = 0; e < un; ++e)
          if (lcc_probe(ot, omask, gdstU[ub + e])) ++hits;
      }
      my_v += hits;
    }
    if (my_v) atomicAdd(&s_hits, my_v);
    __syncthreads();
    if (threadIdx.x == 0 && s_hits) atomicAdd(&T[v], s_hits);
    __syncthreads();
  }
}

// heavy (wave-per-edge, lanes split the enumeration)
__global__ void lcc_dir_heavy_kernel(
    const uint64_t* __restrict__ goffU, const uint32_t* __restrict__ gdstU,
    const uint64_t* __restrict__ hoffU, const uint32_t* __restrict__ htabU,
    const uint64_t* __restrict__ goffO, const uint32_t* __restrict__ gdstO,
    const uint64_t* __restrict__ hoffO, const uint32_t* __restrict__ htabO,
    const unsigned long long* __restrict__ heavy_q, uint64_t heavy_n,
    unsigned long long* __restrict__ T) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid;
       i < heavy_n; i += wstride) {
    unsigned long long pk = heavy_q[i];
    uint32_t v = static_cast<uint32_t>(pk >> 32);
    uint32_t u = static_cast<uint32_t>(pk);
    uint64_t ub = goffU[v];
    uint32_t un = static_cast<uint32_t>(goffU[v + 1] - ub);
    uint64_t ob = goffO[u];
    uint32_t on = static_cast<uint32_t>(goffO[u + 1] - ob);
    unsigned long long hits = 0;
    if (on <= un) {
      const uint64_t mask = (hoffU[v + 1] - hoffU[v]) - 1;
      const uint32_t* t = htabU + hoffU[v];
      for (uint32_t e = lane; e < on; e += kWave)
        if (lcc_probe(t, mask, gdstO[ob + e])) ++hits;
    } else {
      const uint64_t mask = (hoffO[u + 1] - hoffO[u]) - 1;
      const uint32_t* t = htabO + hoffO[u];
      for (uint32_t e = lane; e < un; e += kWave)
        if (lcc_probe(t, mask, gdstU[ub + e])) ++hits;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
      hits += __shfl_down(hits, d, 64);
    if (lane == 0 && hits) atomicAdd(&T[v], hits);
  }
}

// caps for the dedup'd OUT family: distinct-out <= min(out_deg, D)
__global__ void lcc_outcap_kernel(const uint64_t* __restrict__ off,
                                  const uint32_t* __restrict__ D,
                                  uint32_t owned, uint32_t v_begin,
                                  uint32_t* __restrict__ caps) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride) {
    uint64_t d = off[r + 1] - off[r];
    uint32_t dd = D[v_begin + r];
    caps[r] = static_cast<uint32_t>(d < dd ? d : dd);
  }
}

// lcc = scale * T / (D (D - 1)): scale 2.0 undirected (T = triangles at v,
// over unordered neighbor pairs), 1.0 directed (T = arcs among N(v), over
// ordered pairs)
__global__ void lcc_finalize_kernel(const unsigned long long* __restrict__ T,
                                    const uint32_t* __restrict__ D,
                                    uint32_t owned, uint32_t v_begin,
                                    double scale, double* __restrict__ lcc) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < owned;
       r += stride) {
    uint32_t d = D[v_begin + r];
    lcc[r] = d < 2 ? 0.0
                   : scale * static_cast<double>(T[v_begin + r]) /
                         (static_cast<double>(d) * (d - 1));
  }
}

namespace {

// mark remote dsts of the capacity-layout oriented adjacency (wave/row)
__global__ void lcc_mark_oriented_kernel(
    const uint64_t* __restrict__ ooff, const uint32_t* __restrict__ ocnt,
    const uint32_t* __restrict__ oadj, uint32_t owned, uint32_t v_begin,
    uint32_t v_end, DevBitmap bm) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid;
       i < owned; i += wstride) {
    uint64_t b = ooff[i];
    uint32_t n = ocnt[i];
    for (uint32_t k = lane; k < n; k += kWave) {
      uint32_t v = oadj[b + k];
      if (v < v_begin || v >= v_end) (void)bm.set_once(v);
    }
  }
}

// pack requested rows (sorted, variable length) into a contiguous payload
__global__ void lcc_pack_rows_kernel(const uint32_t* __restrict__ idx,
                                     uint64_t n,
                                     const uint64_t* __restrict__ goff,
                                     const uint32_t* __restrict__ gdst,
                                     const uint64_t* __restrict__ pack_off,
                                     uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wpb = kBlock / kWave;
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * wpb + wid; i < n;
       i += wstride) {
    uint64_t b = goff[idx[i]];
    uint64_t o = pack_off[i], len = pack_off[i + 1] - o;
    for (uint64_t k = lane; k < len; k += kWave) out[o + k] = gdst[b + k];
  }
}

struct GlobalDedupCsr {
  DeviceBuffer<uint32_t> gcnt;
  DeviceBuffer<uint64_t> goff;
  DeviceBuffer<uint32_t> gdst;
  uint64_t total = 0;
};

// Fetch the referenced remote rows of a sparse-count CSR: each owner
// packs exactly the rows each peer requested (sidx/soff lists); payloads
// land directly in the requester's contiguous per-owner gdst regions
// (unfetched rows have zero count, so regions are hole-free). Counts
// must already be synced over the same lists.
void lcc_fetch_referenced_rows(GpuContext::Impl& I,
                               const DeviceBuffer<uint32_t>& sidx,
                               const std::vector<uint64_t>& soff,
                               const DeviceBuffer<uint32_t>& gcnt,
                               const DeviceBuffer<uint64_t>& goff,
                               DeviceBuffer<uint32_t>& gdst, uint32_t slice,
                               uint32_t nv_pad, int world, hipStream_t s) {
  uint64_t ns = soff[world];
  DeviceBuffer<uint32_t> slen(ns ? ns : 1);
  if (ns)
    gather4_kernel<<<grid_for(ns), kBlock, 0, s>>>(sidx.data(), ns,
                                                   gcnt.data(), slen.data());
  DeviceBuffer<uint64_t> spack(ns + 1);
  uint64_t stotal = exclusive_scan(slen.data(), spack.data(), ns, s, I.scan);
  DeviceBuffer<uint32_t> srows(stotal ? stotal : 1);
  if (ns)
    lcc_pack_rows_kernel<<<grid_for(ns * kWave), kBlock, 0, s>>>(
        sidx.data(), ns, goff.data(), gdst.data(), spack.data(),
        srows.data());
  // per-peer byte offsets: send = packed scan at list boundaries,
  // recv = goff at slice boundaries (both derive from the same counts)
  std::vector<uint64_t> sb(world + 1), rb(world + 1);
  for (int f = 0; f <= world; ++f) {
    uint64_t v = 0;
    HIP_CHECK(hipMemcpyAsync(&v, spack.data() + soff[f], 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    sb[f] = v * 4;
    uint64_t idx =
        std::min<uint64_t>(static_cast<uint64_t>(f) * slice, nv_pad);
    HIP_CHECK(hipMemcpyAsync(&v, goff.data() + idx, 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    rb[f] = v * 4;
  }
  I.dc.sendrecv(reinterpret_cast<const uint8_t*>(srows.data()), sb,
                reinterpret_cast<uint8_t*>(gdst.data()), rb, s);
  HIP_CHECK(hipStreamSynchronize(s));
}

// --- set-building helpers, in call order: tiers -> distinct -> emit ->
// global CSR -> hash sets ------------------------------------------------

// The shared combined-degree tiers (no tiny tier: those rows are small
// rows) plus LCC's table pool for the large tier: u32 labels, cleared
// before each pass.
struct LccTiers : RowTiers {
  DeviceBuffer<uint32_t> tbl_lab;
};

LccTiers build_lcc_tiers(GpuContext::Impl& I, const uint64_t* off1,
                         const uint64_t* off2, uint32_t owned,
                         hipStream_t s) {
  LccTiers t{build_row_tiers(off1, off2, owned, false, s, I.scan), {}};
  t.tbl_lab.resize(t.heavy_total);
  return t;
}

// one dedup pass of (o1,d1[,o2,d2]) over all four tiers into `sink`
template <typename Sink>
void launch_dedup_tiers(LccTiers& t, const uint64_t* o1, const uint32_t* d1,
                        const uint64_t* o2, const uint32_t* d2,
                        uint32_t v_begin, Sink sink, hipStream_t s) {
  if (t.n_small)
    lcc_dedup_small_kernel<<<grid_for(t.n_small * kWave), kBlock, 0, s>>>(
        o1, d1, o2, d2, t.small.data(), t.n_small, v_begin, sink);
  if (t.n_wave)
    lcc_dedup_wave_kernel<<<grid_for(((t.n_wave + 3) / 4) * kBlock), kBlock,
                            0, s>>>(o1, d1, o2, d2, t.wave.data(), t.n_wave,
                                    v_begin, sink);
  if (t.n_mid)
    lcc_dedup_mid_kernel<<<std::min<int>(t.n_mid, kMaxGrid), kBlock, 0, s>>>(
        o1, d1, o2, d2, t.mid.data(), t.n_mid, v_begin, sink);
  if (t.n_large) {
    fill(t.tbl_lab.data(), kSlotEmpty, t.heavy_total, s);
    lcc_dedup_large_kernel<<<std::min<int>(t.n_large, kMaxGrid), kBlock, 0,
                             s>>>(o1, d1, o2, d2, t.large.data(), t.n_large,
                                  t.heavy_off.data(), t.tbl_lab.data(),
                                  v_begin, sink);
  }
}

// Dv[v] = |distinct neighbors of v, excl. self| for owned v (global index).
// Multi: the emit filter reads Dv[dst] for local dsts only, so referenced
// entries are refreshed point-to-point instead of allgathering slices.
void lcc_degree_pass(GpuContext::Impl& I, DeviceGraph& g, LccTiers& t,
                       const uint64_t* o1, const uint32_t* d1,
                       const uint64_t* o2, const uint32_t* d2,
                       uint32_t nv_pad, bool multi,
                       DeviceBuffer<uint32_t>& Dv, hipStream_t s) {
  Dv.resize(nv_pad);
  Dv.zero(s);
  launch_dedup_tiers(t, o1, d1, o2, d2, g.v_begin, LccCountSink{Dv.data()},
                     s);
  if (multi) {
    mirror_sync_begin(I, g, Dv.data(), s);
    mirror_sync_end(I, g, Dv.data(), s);
  }
}

// per-owned-row lists in capacity layout: row r holds ocnt[r] entries at
// oadj[ooff[r]..], with room for caps[r]
struct CapRows {
  DeviceBuffer<uint64_t> ooff;
  DeviceBuffer<uint32_t> oadj, ocnt;
};

// Deduped neighbor lists of (o1,d1[,o2,d2]) in capacity layout; `filter`
// keeps only the oriented side, (D[u],u) > (D[v],v). The tiers may come
// from a wider family (directed O reuses the combined-degree tiers): a row
// only has to fit the tier it sits in.
CapRows lcc_emit_pass(GpuContext::Impl& I, LccTiers& t, const uint64_t* o1,
                      const uint32_t* d1, const uint64_t* o2,
                      const uint32_t* d2, const DeviceBuffer<uint32_t>& caps,
                      bool filter, const DeviceBuffer<uint32_t>& Dv,
                      uint32_t owned, uint32_t v_begin, hipStream_t s) {
  CapRows rows;
  rows.ooff.resize(owned + 1);
  uint64_t cap_total =
      exclusive_scan(caps.data(), rows.ooff.data(), owned, s, I.scan);
  rows.oadj.resize(cap_total ? cap_total : 1);
  rows.ocnt.resize(owned ? owned : 1);
  rows.ocnt.zero(s);
  launch_dedup_tiers(t, o1, d1, o2, d2, v_begin,
                     LccEmitSink{Dv.data(), rows.ooff.data(),
                                 rows.oadj.data(), rows.ocnt.data(), filter},
                     s);
  return rows;
}

// Compact a capacity-layout family into a sparse global-index CSR, taking
// the rows over so oadj is gone before any sort scratch or fetch staging
// is allocated. sort_owned sorts the owned rows ascending before peers
// fetch them. With lists (multi): counts are synced over the request lists
// and referenced remote rows fetched (volume scales with the boundary).
// Without lists: own rows only — for families that are never probed at
// remote indices (directed U, read only at owned v).
void build_global_csr(GpuContext::Impl& I, int world, uint32_t nv_pad,
                      uint32_t slice, uint32_t owned, uint32_t v_begin,
                      CapRows rows, bool sort_owned, GlobalDedupCsr& out,
                      hipStream_t s,
                      const DeviceBuffer<uint32_t>* ridx = nullptr,
                      const std::vector<uint64_t>* roff = nullptr,
                      const DeviceBuffer<uint32_t>* sidx = nullptr,
                      const std::vector<uint64_t>* soff = nullptr) {
  bool fetch = world > 1 && ridx;
  out.gcnt.resize(nv_pad);
  out.gcnt.zero(s);
  HIP_CHECK(hipMemcpyAsync(out.gcnt.data() + v_begin, rows.ocnt.data(),
                           owned * 4, hipMemcpyDeviceToDevice, s));
  if (fetch) {
    // unfetched rows keep a zero count, so they scan to zero length and
    // the fetch regions stay contiguous per owner
    DeviceBuffer<uint8_t> ss((*soff)[world] * 4 + 4),
        sr(roff->back() * 4 + 4);
    ref_sync_begin(I, *sidx, *soff, *roff, ss, sr, out.gcnt.data(), s);
    ref_sync_end(I, *ridx, *roff, sr, out.gcnt.data(), s);
  }
  out.goff.resize(static_cast<size_t>(nv_pad) + 1);
  out.total =
      exclusive_scan(out.gcnt.data(), out.goff.data(), nv_pad, s, I.scan);
  out.gdst.resize(out.total ? out.total : 1);
  if (owned)
    lcc_compact_kernel<<<grid_for(static_cast<size_t>(owned) * kWave),
                         kBlock, 0, s>>>(rows.ooff.data(), rows.ocnt.data(),
                                         rows.oadj.data(), out.goff.data(),
                                         owned, v_begin, out.gdst.data());
  rows.oadj.free();
  if (sort_owned)
    segmented_sort_rows(out.goff.data() + v_begin, owned,
                        U32KeyCodec{out.gdst.data()}, s, I.scan);
  if (fetch)
    lcc_fetch_referenced_rows(I, *sidx, *soff, out.gcnt, out.goff,
                              out.gdst, slice, nv_pad, world, s);
}

// The degree-oriented CSR of an undirected graph, shared by lcc and kclique:
// Dv (distinct degree by global index) and O, the deduplicated rows
// O(v) = {u in N(v) : (D[u], u) > (D[v], v)}, ascending. Multi-GPU holds a
// PARTIAL oriented CSR: own rows + the remote rows local oriented edges name
// (reference TransferAdjList staging, cuda/lcc/lcc.h:490-496, recast as a
// one-shot referenced-row fetch), so memory and exchange volume scale with
// the boundary, not with V. Fetched rows arrive
// sorted: owners sort before peers fetch. The caller has ensured the
// mirrors (multi) and opened its run bracket.
void build_oriented_csr(GpuContext::Impl& I, TcpComm* comm, DeviceGraph& g,
                        int rank, int world, DeviceBuffer<uint32_t>& Dv,
                        GlobalDedupCsr& O, hipStream_t s) {
  uint32_t nv_pad = padded_nv(g, world);
  uint32_t owned = g.owned();
  uint32_t slice = nv_pad / (world ? world : 1);
  bool multi = world > 1;
  const uint64_t* off1 = g.oe_off.data();
  const uint32_t* dst1 = g.oe_dst.data();
  // referenced-row request lists
  DeviceBuffer<uint32_t> ridx, sidx;
  std::vector<uint64_t> roff, soff;

  LccTiers tiers = build_lcc_tiers(I, off1, nullptr, owned, s);
  lcc_degree_pass(I, g, tiers, off1, dst1, nullptr, nullptr, nv_pad, multi,
                  Dv, s);

  // oriented adjacency O(v) in capacity layout (cap = D per row)
  DeviceBuffer<uint32_t> dcap(owned ? owned : 1);
  HIP_CHECK(hipMemcpyAsync(dcap.data(), Dv.data() + g.v_begin, owned * 4,
                           hipMemcpyDeviceToDevice, s));
  CapRows rows = lcc_emit_pass(I, tiers, off1, dst1, nullptr, nullptr, dcap,
                               true, Dv, owned, g.v_begin, s);
  // request the rows local oriented edges reference
  if (multi) {
    size_t nwords = (static_cast<size_t>(nv_pad) + 31) / 32;
    DeviceBuffer<uint32_t> bm(nwords);
    bm.zero(s);
    if (owned)
      lcc_mark_oriented_kernel<<<grid_for(static_cast<size_t>(owned) * kWave),
                                 kBlock, 0, s>>>(
          rows.ooff.data(), rows.ocnt.data(), rows.oadj.data(), owned,
          g.v_begin, g.v_end, DevBitmap{bm.data()});
    build_ref_lists(I, comm, bm, nwords, slice, rank, world, ridx, roff,
                    sidx, soff, s);
  }
  // owners sort their rows before peers fetch them
  build_global_csr(I, world, nv_pad, slice, owned, g.v_begin, std::move(rows),
                   true, O, s, multi ? &ridx : nullptr,
                   multi ? &roff : nullptr, multi ? &sidx : nullptr,
                   multi ? &soff : nullptr);
}

// per-vertex open-addressing sets over a global CSR (capacity 2x, pow2)
void build_hash_sets(GpuContext::Impl& I, uint32_t nv_pad,
                     const GlobalDedupCsr& csr, DeviceBuffer<uint64_t>& hoff,
                     DeviceBuffer<uint32_t>& htab, hipStream_t s) {
  DeviceBuffer<uint32_t> hcap(nv_pad);
  hoff.resize(static_cast<size_t>(nv_pad) + 1);
  lcc_hashcap_kernel<<<grid_for(nv_pad), kBlock, 0, s>>>(csr.goff.data(),
                                                         nv_pad,
                                                         hcap.data());
  uint64_t total = exclusive_scan(hcap.data(), hoff.data(), nv_pad, s,
                                  I.scan);
  hcap.free();
  htab.resize(total);
  fill(htab.data(), kSlotEmpty, total, s);
  lcc_hashfill_kernel<<<grid_for(static_cast<size_t>(nv_pad) * kWave),
                        kBlock, 0, s>>>(csr.goff.data(), csr.gdst.data(),
                                        hoff.data(), nv_pad, htab.data());
}

// --- counting tail shared by both variants ------------------------------
// begin: credits T, the deferred-edge queue, and the owned rows of `goff`
// bucketed into the two light tiers. The caller launches its own light
// kernels, reads the queue length back with lcc_heavy_count, launches its
// heavy kernel, and ends with lcc_finish.
struct LccTail {
  DeviceBuffer<unsigned long long> Tcnt;
  uint32_t heavy_thresh = 48;
  DeviceBuffer<unsigned long long> heavy_q, heavy_n;
  DeviceBuffer<uint32_t> wee_rows, big_rows;
  uint64_t n_wee = 0, n_big = 0;
};

LccTail lcc_tail_begin(DeviceGraph& g, uint32_t nv_pad,
                       const DeviceBuffer<uint64_t>& goff, uint32_t min_n,
                       hipStream_t s) {
  uint32_t owned = g.owned();
  LccTail t;
  t.Tcnt.resize(nv_pad);
  t.Tcnt.zero(s);
  // min-side size above which an edge defers to the wave-per-edge pass;
  // 96 -> 48 after the two-box sweep + clean full-scale re-measurement
  // (profiles/r01_lcc_heavy_thresh_sweep.md, r02_lcc_heavy48_datagen90:
  // 2.62 s -> 2.50 s)
  if (const char* ht = getenv("GRAPEHIP_LCC_HEAVY"))
    t.heavy_thresh = static_cast<uint32_t>(atoi(ht));
  t.heavy_n.resize(1);
  t.heavy_n.zero(s);
  {
    // worst case: every edge of the owned rows is heavy
    uint64_t lo = 0, hi = 0;
    HIP_CHECK(hipMemcpyAsync(&lo, goff.data() + g.v_begin, 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(
        &hi, goff.data() + std::min<uint64_t>(g.v_end, nv_pad), 8,
        hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    t.heavy_q.resize(std::max<uint64_t>(hi - lo, 1));
  }
  if (owned) {
    auto tc = partition_rows(LccLenTiers{goff.data(), g.v_begin, min_n},
                             owned, {&t.wee_rows, &t.big_rows}, s);
    t.n_wee = tc[0], t.n_big = tc[1];
  }
  return t;
}

// the light kernels are enqueued: drop their row lists and read back how
// many edges they deferred
uint64_t lcc_heavy_count(LccTail& t, hipStream_t s) {
  t.wee_rows.free();
  t.big_rows.free();
  unsigned long long hn = 0;
  HIP_CHECK(hipMemcpyAsync(&hn, t.heavy_n.data(), 8, hipMemcpyDeviceToHost,
                           s));
  HIP_CHECK(hipStreamSynchronize(s));
  return hn;
}

GpuRunResult lcc_finish(const RunBracket& br, DeviceGraph& g,
                        const LccTail& t, const DeviceBuffer<uint32_t>& Dv,
                        double scale, bool fetch, hipStream_t s) {
  uint32_t owned = g.owned();
  DeviceBuffer<double> lcc_out(owned ? owned : 1);
  if (owned)
    lcc_finalize_kernel<<<grid_for(owned), kBlock, 0, s>>>(
        t.Tcnt.data(), Dv.data(), owned, g.v_begin, scale, lcc_out.data());
  GpuRunResult res = br.finish(1, g.input_edges);
  if (fetch) {
    res.f64.resize(owned);
    HIP_CHECK(hipMemcpyAsync(res.f64.data(), lcc_out.data(), owned * 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  return res;
}

}  // namespace

// Directed LCC: build the union family U(v)=N(v) and the deduped OUT
// family Nout(v), then count |U(v) ∩ Nout(u)| per (v, u∈U(v)) pair.
GpuRunResult GpuContext::lcc_directed(DeviceGraph& g, bool fetch) {
  RangeMarker _mk("grapehip::lcc_directed");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  uint32_t slice = nv_pad / (world_ ? world_ : 1);
  bool multi = world_ > 1;
  if (!g.has_in)
    throw std::runtime_error(
        "GPU directed LCC needs the in-CSR (build_in_csr=True)");
  const uint64_t* off1 = g.oe_off.data();
  const uint32_t* dst1 = g.oe_dst.data();
  const uint64_t* off2 = g.ie_off.data();
  const uint32_t* dst2 = g.ie_dst.data();

  // referenced-row request lists (multi): only the O family is probed at
  // remote indices (kernels read U solely at owned v), so U stays local
  // and O rows are fetched for the u's own U rows actually name
  DeviceBuffer<uint32_t> ridx, sidx;
  std::vector<uint64_t> roff, soff;
  if (multi) ensure_mirrors(I, comm_, g, rank_, world_, s);

  RunBracket br(I, comm_);

  DeviceBuffer<uint32_t> Dv;
  GlobalDedupCsr U, O;
  {
    // both families run over the tiers of the combined in+out degree
    LccTiers tiers = build_lcc_tiers(I, off1, off2, owned, s);
    lcc_degree_pass(I, g, tiers, off1, dst1, off2, dst2, nv_pad, multi, Dv,
                      s);

    // U family: in ∪ out, cap = D — never probed remotely, stays local
    {
      DeviceBuffer<uint32_t> caps(owned ? owned : 1);
      HIP_CHECK(hipMemcpyAsync(caps.data(), Dv.data() + g.v_begin,
                               owned * 4, hipMemcpyDeviceToDevice, s));
      build_global_csr(I, world_, nv_pad, slice, owned, g.v_begin,
                       lcc_emit_pass(I, tiers, off1, dst1, off2, dst2, caps,
                                     false, Dv, owned, g.v_begin, s),
                       false, U, s);
    }
    // referenced u's = dsts of own U rows (the only rows whose O family
    // the count kernels probe)
    if (multi) {
      uint64_t ub = 0, ue = 0;
      HIP_CHECK(hipMemcpyAsync(&ub, U.goff.data() + g.v_begin, 8,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&ue,
                               U.goff.data() + std::min<uint64_t>(
                                   g.v_end, nv_pad),
                               8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      size_t nwords = (static_cast<size_t>(nv_pad) + 31) / 32;
      DeviceBuffer<uint32_t> bm(nwords);
      bm.zero(s);
      if (ue > ub)
        mark_dsts_kernel<<<grid_for(ue - ub), kBlock, 0, s>>>(
            U.gdst.data() + ub, ue - ub, g.v_begin, g.v_end,
            DevBitmap{bm.data()});
      build_ref_lists(I, comm_, bm, nwords, slice, rank_, world_, ridx,
                      roff, sidx, soff, s);
    }
    // O family: distinct out, cap = min(out_deg, D)
    {
      DeviceBuffer<uint32_t> caps(owned ? owned : 1);
      if (owned)
        lcc_outcap_kernel<<<grid_for(owned), kBlock, 0, s>>>(
            off1, Dv.data(), owned, g.v_begin, caps.data());
      build_global_csr(I, world_, nv_pad, slice, owned, g.v_begin,
                       lcc_emit_pass(I, tiers, off1, dst1, nullptr, nullptr,
                                     caps, false, Dv, owned, g.v_begin, s),
                       false, O, s, multi ? &ridx : nullptr,
                       multi ? &roff : nullptr, multi ? &sidx : nullptr,
                       multi ? &soff : nullptr);
    }
  }

  DeviceBuffer<uint64_t> hoffU, hoffO;
  DeviceBuffer<uint32_t> htabU, htabO;
  build_hash_sets(I, nv_pad, U, hoffU, htabU, s);
  build_hash_sets(I, nv_pad, O, hoffO, htabO, s);

  LccTail t = lcc_tail_begin(g, nv_pad, U.goff, 2, s);
  if (t.n_wee)
    lcc_dir_count_wee_kernel<<<grid_for(t.n_wee * kWave), kBlock, 0, s>>>(
        U.goff.data(), U.gdst.data(), hoffU.data(), htabU.data(),
        O.goff.data(), O.gdst.data(), hoffO.data(), htabO.data(),
        t.wee_rows.data(), t.n_wee, g.v_begin, t.Tcnt.data(), t.heavy_thresh,
        t.heavy_q.data(), t.heavy_n.data());
  if (t.n_big)
    lcc_dir_count_staged_kernel<<<std::min<uint64_t>(t.n_big, kMaxGrid),
                                  kBlock, 0, s>>>(
        U.goff.data(), U.gdst.data(), hoffU.data(), htabU.data(),
        O.goff.data(), O.gdst.data(), hoffO.data(), htabO.data(),
        t.big_rows.data(), t.n_big, g.v_begin, t.Tcnt.data(), t.heavy_thresh,
        t.heavy_q.data(), t.heavy_n.data());
  uint64_t hn = lcc_heavy_count(t, s);
  if (hn)
    lcc_dir_heavy_kernel<<<grid_for(hn * kWave), kBlock, 0, s>>>(
        U.goff.data(), U.gdst.data(), hoffU.data(), htabU.data(),
        O.goff.data(), O.gdst.data(), hoffO.data(), htabO.data(),
        t.heavy_q.data(), hn, t.Tcnt.data());
  return lcc_finish(br, g, t, Dv, 1.0, fetch, s);
}

GpuRunResult GpuContext::lcc(DeviceGraph& g, bool fetch) {
  RangeMarker _mk("grapehip::lcc");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  uint32_t nv_pad = padded_nv(g, world_);
  bool multi = world_ > 1;
  if (g.directed) return lcc_directed(g, fetch);

  // graph-sized working set (freed on return)
  DeviceBuffer<uint32_t> Dv;  // distinct degree, global idx
  GlobalDedupCsr O;           // oriented CSR (own + referenced rows), sorted
  if (multi) ensure_mirrors(I, comm_, g, rank_, world_, s);

  RunBracket br(I, comm_);

  build_oriented_csr(I, comm_, g, rank_, world_, Dv, O, s);

  // per-vertex oriented hash sets (intersection via O(1) probes)
  DeviceBuffer<uint64_t> hoff;
  DeviceBuffer<uint32_t> htab;
  build_hash_sets(I, nv_pad, O, hoff, htab, s);

  // triangle counting: light edges inline, heavy edges deferred to a
  // wave-per-edge pass (power-law tail otherwise stalls single lanes)
  const bool nowit = getenv("GRAPEHIP_LCC_NOWIT") != nullptr;
  LccTail t = lcc_tail_begin(g, nv_pad, O.goff, 1, s);
  if (t.n_wee)
    lcc_tri_wee_kernel<<<grid_for(t.n_wee * kWave), kBlock, 0, s>>>(
        O.goff.data(), O.gdst.data(), hoff.data(), htab.data(),
        t.wee_rows.data(), t.n_wee, g.v_begin, t.Tcnt.data(), t.heavy_thresh,
        t.heavy_q.data(), t.heavy_n.data(), nowit);
  if (t.n_big)
    lcc_tri_staged_kernel<<<std::min<uint64_t>(t.n_big, kMaxGrid), kBlock, 0,
                            s>>>(
        O.goff.data(), O.gdst.data(), hoff.data(), htab.data(),
        t.big_rows.data(), t.n_big, g.v_begin, t.Tcnt.data(), t.heavy_thresh,
        t.heavy_q.data(), t.heavy_n.data(), nowit);
  uint64_t hn = lcc_heavy_count(t, s);
  if (getenv("GRAPEHIP_DEBUG"))
    fprintf(stderr, "[lcc] oriented_total=%llu heavy_edges=%llu\n",
            static_cast<unsigned long long>(O.total),
            static_cast<unsigned long long>(hn));
  if (hn)
    lcc_triangle_heavy_kernel<<<grid_for(hn * kWave), kBlock, 0, s>>>(
        O.goff.data(), O.gdst.data(), hoff.data(), htab.data(),
        t.heavy_q.data(), hn, t.Tcnt.data());
  if (multi) I.dc.allreduce_sum_u64(t.Tcnt.data(), nv_pad, s);
  return lcc_finish(br, g, t, Dv, 2.0, fetch, s);
}

// ---------------------------------------------------------------------------
// k-clique counting: bitmap enumeration over the oriented CSR (KERNELS.md
// "k-clique bitmap enumeration"). Every vertex of a clique rooted at an owned
// v (its lowest vertex in (D, id) order) lies in O(v), so per row the induced
// DAG on O(v) = u_0..u_{d-1} is a d x ceil(d/64) bit matrix, bit (i, j) set
// iff u_j is in O(u_i), and the (k-1)-cliques of that DAG are counted by
// bitset recursion: cand_1 = adj[i], cand_{t+1} = cand_t & adj[j] for each
// j in cand_t, popc(cand) once k-1 vertices are fixed. The orientation is
// acyclic, so each clique is met once.
// ---------------------------------------------------------------------------

#ifndef GRAPEHIP_KCLIQUE_BLOCK_MAX
#define GRAPEHIP_KCLIQUE_BLOCK_MAX 512
#endif
// Largest d whose matrix is staged in LDS, one block per row: 512^2 bits are
// 32 KiB (four blocks per CU), 1024^2 bits 128 KiB (one). Measured in
// profiles/r10_gpu_kclique.md.
constexpr uint32_t kCliqueBlockMax = GRAPEHIP_KCLIQUE_BLOCK_MAX;
static_assert(kCliqueBlockMax >= 128 && kCliqueBlockMax <= 1024 &&
                  kCliqueBlockMax % 64 == 0,
              "block tier: 2 to 16 mask words per row");
// global tier: one wave per DFS, up to 16 mask words per lane
constexpr uint32_t kCliqueMaxWpl = 16;
constexpr uint32_t kCliqueMaxDeg = kWave * 64 * kCliqueMaxWpl;  // 65536
// HBM workspace of the global tier: at most this, or one slab if larger
constexpr uint64_t kCliqueWorkspaceBytes = 1ull << 30;
constexpr int kCliqueGlobalBlocksPerCu = 2;
constexpr uint32_t kCliqueNone = 0xFFFFFFFFu;

// one candidate set, spread over a group of G lanes: lane l of the group
// holds words l, l + G, l + 2G, ...
template <int WPL>
struct KcMask {
  unsigned long long w[WPL];
};

// lowest member of the group's set above `prev` (-1: lowest of all), the
// same value in every lane of the group; kCliqueNone when there is none.
// All lanes of a group call this together.
template <int G, int WPL>
__device__ __forceinline__ uint32_t kc_next(const KcMask<WPL>& c,
                                            uint32_t lane_g, int prev) {
  const int pw = prev >> 6;  // -1 for prev == -1
  const int pb = prev & 63;
  uint32_t mine = kCliqueNone;
#pragma unroll
  for (int q = WPL - 1; q >= 0; --q) {  // descending: the lowest word wins
    const int wi = static_cast<int>(lane_g) + G * q;
    unsigned long long x = c.w[q];
    if (wi < pw)
      x = 0;
    else if (wi == pw)
      x = pb == 63 ? 0ull : x & (~0ull << (pb + 1));
    if (x) mine = static_cast<uint32_t>(wi) * 64 + (__ffsll(x) - 1);
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    uint32_t other = __shfl_xor(mine, o, 64);
    mine = other < mine ? other : mine;
  }
  return mine;
}

// Cliques below `cand` with `need` more vertices to fix before the leaf;
// each lane returns the share of its own words. LEFT bounds the recursion at
// compile time, so the mask stack lives in registers.
template <int G, int WPL, int LEFT>
__device__ __forceinline__ unsigned long long kc_dfs(
    const unsigned long long* adj, uint32_t W, uint32_t lane_g,
    const KcMask<WPL>& cand, int need) {
  unsigned long long t = 0;
  if (need == 0) {
#pragma unroll
    for (int q = 0; q < WPL; ++q) t += __popcll(cand.w[q]);
    return t;
  }
  if constexpr (LEFT > 0) {
    int prev = -1;
    for (;;) {
      uint32_t j = kc_next<G, WPL>(cand, lane_g, prev);
      if (j == kCliqueNone) break;
      prev = static_cast<int>(j);
      const unsigned long long* row = adj + static_cast<size_t>(j) * W;
      KcMask<WPL> nxt;
#pragma unroll
      for (int q = 0; q < WPL; ++q) {
        uint32_t wi = lane_g + G * q;
        nxt.w[q] = wi < W ? cand.w[q] & row[wi] : 0ull;
      }
      t += kc_dfs<G, WPL, LEFT - 1>(adj, W, lane_g, nxt, need - 1);
    }
  }
  return t;
}

// The groups of a block take the sub-roots i of one row from a shared
// counter (balance: the subtrees differ widely); each runs the DFS below
// cand_1 = adj[i].
template <int G, int WPL>
__device__ __forceinline__ unsigned long long kc_group_roots(
    const unsigned long long* adj, uint32_t d, uint32_t W, uint32_t* next,
    int need) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t lane_g = lane & (G - 1);
  unsigned long long t = 0;
  for (;;) {
    uint32_t i = 0;
    if (lane_g == 0) i = atomicAdd(next, 1u);
    i = __shfl(i, static_cast<int>(lane - lane_g), 64);
    if (i >= d) break;
    const unsigned long long* row = adj + static_cast<size_t>(i) * W;
    KcMask<WPL> cand;
#pragma unroll
    for (int q = 0; q < WPL; ++q) {
      uint32_t wi = lane_g + G * q;
      cand.w[q] = wi < W ? row[wi] : 0ull;
    }
    t += kc_dfs<G, WPL, kCliqueMaxK - 3>(adj, W, lane_g, cand, need);
  }
  return t;
}

// bit (i, j) for every w = u_j of O(u_i) found in the sorted nbr[0..d): the
// block's waves stride the rows i, the lanes of a wave the entries of O(u_i).
// adj is zeroed and the writes are visible to the block.
__device__ __forceinline__ void kc_build_matrix(
    const uint64_t* __restrict__ goff, const uint32_t* __restrict__ gdst,
    const uint32_t* nbr, uint32_t d, uint32_t W, unsigned long long* adj) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wpb = blockDim.x >> 6;
  for (uint32_t i = threadIdx.x >> 6; i < d; i += wpb) {
    uint32_t u = nbr[i];
    uint64_t ub = goff[u];
    uint32_t un = static_cast<uint32_t>(goff[u + 1] - ub);
    for (uint32_t e = lane; e < un; e += kWave) {
      uint32_t w = gdst[ub + e];
      uint32_t lo = 0, hi = d;
      while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if (nbr[mid] < w)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < d && nbr[lo] == w)
        atomicOr(&adj[static_cast<size_t>(i) * W + (lo >> 6)],
                 1ull << (lo & 63));
    }
  }
}

__device__ __forceinline__ void kc_add_total(unsigned long long t,
                                             unsigned long long* total) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
  if ((threadIdx.x & 63) == 0 && t) atomicAdd(total, t);
}

// wave tier (d <= 64): one wave per row, lane i owns u_i and matrix row i.
// Row i is one ballot: lane j searches u_j in the sorted O(u_i). The words
// are parked in LDS per wave for the DFS, where lane i walks the subtree of
// sub-root i alone (G = 1: no cross-lane traffic).
__global__ __launch_bounds__(kBlock) void kclique_wave_kernel(
    const uint64_t* __restrict__ goff, const uint32_t* __restrict__ gdst,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    int need, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_adj[kBlock / kWave][kWave];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wid = threadIdx.x >> 6;
  const uint32_t wpb = kBlock / kWave;
  unsigned long long* adj = s_adj[wid];
  size_t wstride = static_cast<size_t>(gridDim.x) * wpb;
  unsigned long long t = 0;
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * wpb + wid; r < nrows;
       r += wstride) {
    uint32_t v = v_begin + rows[r];
    uint64_t vb = goff[v];
    uint32_t d = static_cast<uint32_t>(goff[v + 1] - vb);  // <= 64
    uint32_t mine = lane < d ? gdst[vb + lane] : 0;
    unsigned long long my_row = 0;
    for (uint32_t i = 0; i < d; ++i) {
      uint32_t u = __shfl(mine, static_cast<int>(i), 64);
      uint64_t ub = goff[u];
      uint32_t lo = 0, hi = static_cast<uint32_t>(goff[u + 1] - ub);
      const uint32_t un = hi;
      bool hit = false;
      if (lane < d) {
        while (lo < hi) {
          uint32_t mid = (lo + hi) >> 1;
          if (gdst[ub + mid] < mine)
            lo = mid + 1;
          else
            hi = mid;
        }
        hit = lo < un && gdst[ub + lo] == mine;
      }
      unsigned long long word = __ballot(hit);
      if (lane == i) my_row = word;
    }
    // the wave's own LDS traffic is ordered; the fences keep the compiler
    // from moving the DFS reads above the store (and the next row's store
    // above this row's reads)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    adj[lane] = my_row;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < d) {
      KcMask<1> cand{{my_row}};
      t += kc_dfs<1, 1, kCliqueMaxK - 3>(adj, 1, 0, cand, need);
    }
  }
  kc_add_total(t, total);
}

// block tier (64 < d <= kCliqueBlockMax): one block per row, O(v) and the
// matrix staged in LDS, the matrix built with LDS atomicOr. Groups of G =
// W rounded up to a power of two lanes own one DFS each, one word per lane.
__global__ __launch_bounds__(kBlock) void kclique_block_kernel(
    const uint64_t* __restrict__ goff, const uint32_t* __restrict__ gdst,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    int need, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_adj[kCliqueBlockMax * (kCliqueBlockMax / 64)];
  __shared__ uint32_t s_nbr[kCliqueBlockMax];
  __shared__ uint32_t s_next;
  unsigned long long t = 0;
  for (uint64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    uint32_t v = v_begin + rows[r];
    uint64_t vb = goff[v];
    uint32_t d = static_cast<uint32_t>(goff[v + 1] - vb);
    uint32_t W = (d + 63) >> 6;  // 2..kCliqueBlockMax/64
    for (uint32_t x = threadIdx.x; x < d; x += blockDim.x)
      s_nbr[x] = gdst[vb + x];
    for (uint32_t x = threadIdx.x; x < d * W; x += blockDim.x) s_adj[x] = 0;
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
    kc_build_matrix(goff, gdst, s_nbr, d, W, s_adj);
    __syncthreads();
    if (W <= 2)
      t += kc_group_roots<2, 1>(s_adj, d, W, &s_next, need);
    else if (W <= 4)
      t += kc_group_roots<4, 1>(s_adj, d, W, &s_next, need);
    else if (W <= 8)
      t += kc_group_roots<8, 1>(s_adj, d, W, &s_next, need);
    else
      t += kc_group_roots<16, 1>(s_adj, d, W, &s_next, need);
    __syncthreads();
  }
  kc_add_total(t, total);
}

// global tier (d > kCliqueBlockMax): persistent blocks, the matrix of the
// row in hand in the block's HBM slab (slab_words, sized by the largest d of
// the tier), O(v) searched where it lies in the CSR. One wave per DFS, WPL
// words per lane (64 * WPL >= W for every row of the tier). The slab is
// reused from row to row and the matrix is written with device atomics, so
// agent-scope fences around the barriers keep a wave from reading the last
// row's lines out of its L1.
template <int WPL>
__global__ __launch_bounds__(kBlock) void kclique_global_kernel(
    const uint64_t* __restrict__ goff, const uint32_t* __restrict__ gdst,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t v_begin,
    int need, unsigned long long* ws, uint64_t slab_words,
    unsigned long long* __restrict__ total) {
  __shared__ uint32_t s_next;
  unsigned long long* adj = ws + static_cast<size_t>(blockIdx.x) * slab_words;
  unsigned long long t = 0;
  for (uint64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    uint32_t v = v_begin + rows[r];
    uint64_t vb = goff[v];
    uint32_t d = static_cast<uint32_t>(goff[v + 1] - vb);
    uint32_t W = (d + 63) >> 6;
    const uint64_t words = static_cast<uint64_t>(d) * W;  // <= slab_words
    for (uint64_t x = threadIdx.x; x < words; x += blockDim.x) adj[x] = 0;
    if (threadIdx.x == 0) s_next = 0;
    __threadfence();
    __syncthreads();
    kc_build_matrix(goff, gdst, gdst + vb, d, W, adj);
    __threadfence();
    __syncthreads();
    __threadfence();
    t += kc_group_roots<kWave, WPL>(adj, d, W, &s_next, need);
    __syncthreads();
  }
  kc_add_total(t, total);
}

namespace {

// rows by oriented out-degree d; rows with d < k - 1 root no k-clique
struct KCliqueTiers {
  static constexpr int kLists = 3, kBins = 3;
  const uint64_t* __restrict__ goff;
  uint32_t v_begin, min_d;
  __device__ __forceinline__ int operator()(uint32_t r) const {
    uint64_t d = goff[v_begin + r + 1] - goff[v_begin + r];
    return d < min_d ? -1 : (d <= kWave ? 0 : (d <= kCliqueBlockMax ? 1 : 2));
  }
};

__global__ void kclique_maxlen_kernel(const uint64_t* __restrict__ goff,
                                      const uint32_t* __restrict__ rows,
                                      uint64_t nrows, uint32_t v_begin,
                                      uint32_t* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nrows;
       i += stride) {
    uint32_t v = v_begin + rows[i];
    uint64_t d = goff[v + 1] - goff[v];
    atomicMax(out, static_cast<uint32_t>(
                       d < 0xFFFFFFFFull ? d : 0xFFFFFFFFull));
  }
}

template <int WPL>
void launch_kclique_global(int grid, hipStream_t s, const GlobalDedupCsr& O,
                           const uint32_t* rows, uint64_t nrows,
                           uint32_t v_begin, int need,
                           unsigned long long* ws, uint64_t slab_words,
                           unsigned long long* total) {
  kclique_global_kernel<WPL><<<grid, kBlock, 0, s>>>(
      O.goff.data(), O.gdst.data(), rows, nrows, v_begin, need, ws,
      slab_words, total);
}

}  // namespace

GpuRunResult GpuContext::kclique(DeviceGraph& g, int k) {
  RangeMarker _mk("grapehip::kclique");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  if (g.directed)
    throw std::runtime_error("GPU kclique: undirected graphs only");
  if (k < 2) throw std::runtime_error("kclique: k must be >= 2");
  if (k > kCliqueMaxK)
    throw std::runtime_error("kclique: k = " + std::to_string(k) +
                             " is above the device limit of " +
                             std::to_string(kCliqueMaxK) + " (kCliqueMaxK)");
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  bool multi = world_ > 1;

  // graph-sized working set (freed on return)
  DeviceBuffer<uint32_t> Dv;
  GlobalDedupCsr O;
  if (multi) ensure_mirrors(I, comm_, g, rank_, world_, s);

  RunBracket br(I, comm_);

  build_oriented_csr(I, comm_, g, rank_, world_, Dv, O, s);
  Dv.free();

  DeviceBuffer<unsigned long long> total(1);
  total.zero(s);
  uint64_t n_tier[3] = {0, 0, 0};
  if (k == 2) {
    // the oriented arcs of the owned rows
    uint64_t lo = 0, hi = 0;
    HIP_CHECK(hipMemcpyAsync(&lo, O.goff.data() + g.v_begin, 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(
        &hi, O.goff.data() + std::min<uint64_t>(g.v_end, nv_pad), 8,
        hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    unsigned long long arcs = hi - lo;
    HIP_CHECK(hipMemcpyAsync(total.data(), &arcs, 8, hipMemcpyHostToDevice,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
  } else if (owned) {
    const int need = k - 3;  // v and the sub-root are fixed
    DeviceBuffer<uint32_t> wave_rows, block_rows, global_rows;
    auto tc = partition_rows(
        KCliqueTiers{O.goff.data(), g.v_begin, static_cast<uint32_t>(k - 1)},
        owned, {&wave_rows, &block_rows, &global_rows}, s);
    for (int b = 0; b < 3; ++b) n_tier[b] = tc[b];
    // the heaviest rows first in flight, the many light ones fill in
    DeviceBuffer<unsigned long long> ws;
    if (n_tier[2]) {
      DeviceBuffer<uint32_t> dmax(1);
      dmax.zero(s);
      kclique_maxlen_kernel<<<grid_for(n_tier[2]), kBlock, 0, s>>>(
          O.goff.data(), global_rows.data(), n_tier[2], g.v_begin,
          dmax.data());
      uint32_t d_max = dmax.download(s)[0];
      if (d_max > kCliqueMaxDeg)
        throw std::runtime_error(
            "kclique: an oriented row of " + std::to_string(d_max) +
            " entries is above the device limit of " +
            std::to_string(kCliqueMaxDeg));
      const uint32_t w_max = (d_max + 63) / 64;
      const uint64_t slab_words = static_cast<uint64_t>(d_max) * w_max;
      uint64_t grid = std::max<uint64_t>(
          1, kCliqueWorkspaceBytes / (slab_words * 8));
      grid = std::min<uint64_t>(
          grid, static_cast<uint64_t>(I.num_cus) * kCliqueGlobalBlocksPerCu);
      grid = std::min<uint64_t>(grid, n_tier[2]);
      ws.resize(grid * slab_words);
      const uint32_t wpl = (w_max + kWave - 1) / kWave;
      auto launch = wpl <= 1   ? launch_kclique_global<1>
                    : wpl <= 2 ? launch_kclique_global<2>
                    : wpl <= 4 ? launch_kclique_global<4>
                    : wpl <= 8 ? launch_kclique_global<8>
                               : launch_kclique_global<16>;
      launch(static_cast<int>(grid), s, O, global_rows.data(), n_tier[2],
             g.v_begin, need, ws.data(), slab_words, total.data());
    }
    if (n_tier[1])
      kclique_block_kernel<<<std::min<uint64_t>(n_tier[1], kMaxGrid), kBlock,
                             0, s>>>(O.goff.data(), O.gdst.data(),
                                     block_rows.data(), n_tier[1], g.v_begin,
                                     need, total.data());
    if (n_tier[0])
      kclique_wave_kernel<<<grid_for(n_tier[0] * kWave), kBlock, 0, s>>>(
          O.goff.data(), O.gdst.data(), wave_rows.data(), n_tier[0],
          g.v_begin, need, total.data());
    HIP_CHECK(hipStreamSynchronize(s));  // the row lists go out of scope
  }
  if (multi) I.dc.allreduce_sum_u64(total.data(), 1, s);
  uint64_t count = total.download(s)[0];
  ++I.kclique_calls;
  for (int b = 0; b < 3; ++b) I.kclique_rows[b] = n_tier[b];
  GpuRunResult res = br.finish(1, g.input_edges);
  res.count = count;
  return res;
}

std::array<uint64_t, 6> GpuContext::debug_kclique(bool reset) {
  auto& I = *impl_;
  std::array<uint64_t, 6> out = {I.kclique_calls, I.kclique_rows[0],
                                 I.kclique_rows[1], I.kclique_rows[2],
                                 kCliqueBlockMax,
                                 static_cast<uint64_t>(kCliqueMaxK)};
  if (reset) {
    I.kclique_calls = 0;
    for (auto& r : I.kclique_rows) r = 0;
  }
  return out;
}

}  // namespace grapehip

namespace grapehip {

// ===========================================================================
// Random-walk sampler (cpp/apps/sampler.hpp on the device). Reference parity:
// examples/gnn_sampler/sampler.h strategies random / edge_weight / top_k
// with per-vertex indexes (fragment_indices.h), recast as walker queues.
//
// One 64-bit draw per step, a function of (seed, walk, hop) alone, so a path
// does not depend on which rank takes the step. A row is the stored out-row
// of the vertex (ascending device id), deg its length:
//   random       pick = hi64(r * deg)
//   edge_weight  cdf = inclusive fp32 prefix sum of the row's weights,
//                t = fp32(r >> 40) * 2^-24 * cdf[deg - 1] (one fp32 multiply),
//                pick = min(deg - 1, #{i : cdf[i] <= t}); a row whose total
//                is not > 0 is a dead end
//   top_k        kk = min(k, deg), pick = the hi64(r * kk)-th arc of the row
//                ordered by weight descending, ties to the smaller slot
// An unweighted graph has every weight 1: edge_weight is then random and
// top_k draws among the first kk slots, with no index.
//
// Walkers are (vertex, walk) pairs in a queue; a step kernel handles one
// walker per lane, writes paths[walk][hop + 1] and appends the walker to the
// next queue (vertex owned) or to the owner's send region, one atomic per
// wave and target. Several ranks: the regions go out with DevComm::sendrecv
// straight into the tail of the receiver's next queue, lengths on the
// control plane; walkers are not deduplicated (two walks may sit on one
// vertex). Every path slot is written by at most one rank over 0xFFFFFFFF,
// so an element-wise min over ranks completes the table at the end.
// ===========================================================================

constexpr uint32_t kSampleThreadDeg = 8;   // thread-per-row index builds
constexpr uint32_t kSampleWaveDeg = 1024;  // wave-per-row; longer: a block
constexpr int kSampleWaveKeys = kSampleWaveDeg / kWave;

struct SampleWalker {
  uint32_t v, walk;
};
static_assert(sizeof(SampleWalker) == 8, "walker queues hold 8-byte entries");

// index-build tiers by row length d: rows of at most min_d arcs have no
// index entry
struct SampleLenTiers {
  static constexpr int kLists = 3, kBins = 3;
  const uint64_t* __restrict__ off;
  uint32_t min_d;
  __device__ __forceinline__ int operator()(uint32_t r) const {
    uint64_t d = off[r + 1] - off[r];
    return d <= min_d ? -1
                      : (d <= kSampleThreadDeg ? 0
                                               : (d <= kSampleWaveDeg ? 1 : 2));
  }
};

__device__ __forceinline__ uint64_t sample_draw(uint64_t seed, uint64_t walk,
                                                uint64_t hop) {
  uint64_t x = seed * 0x9E3779B97F4A7C15ULL + walk * 0xD1B54A32D192ED03ULL +
               hop;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}

__device__ __forceinline__ float wave_incl_scan_f32(float v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    float up = __shfl_up(v, d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), d, 64);
    if (o > v) v = o;
  }
  return v;
}

// --- cdf index: segmented inclusive scan of the weights, three tiers --------

__global__ void sample_cdf_thread_kernel(const uint64_t* __restrict__ off,
                                         const float* __restrict__ w,
                                         const uint32_t* __restrict__ rows,
                                         uint64_t nrows,
                                         float* __restrict__ cdf) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint32_t r = rows[i];
    float acc = 0.f;
    for (uint64_t e = off[r]; e < off[r + 1]; ++e) {
      acc += w[e];
      cdf[e] = acc;
    }
  }
}

__global__ void sample_cdf_wave_kernel(const uint64_t* __restrict__ off,
                                       const float* __restrict__ w,
                                       const uint32_t* __restrict__ rows,
                                       uint64_t nrows,
                                       float* __restrict__ cdf) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nwaves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
  for (uint64_t i = (static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                     threadIdx.x) >> 6;
       i < nrows; i += nwaves) {
    uint32_t r = rows[i];
    const uint64_t b = off[r], e = off[r + 1];
    float carry = 0.f;
    for (uint64_t base = b; base < e; base += kWave) {
      uint64_t idx = base + lane;
      float s = wave_incl_scan_f32(idx < e ? w[idx] : 0.f);
      if (idx < e) cdf[idx] = carry + s;
      carry += __shfl(s, 63, 64);
    }
  }
}

// hub rows: a block scans kBlock arcs at a time and carries the running
// total from chunk to chunk
__global__ void __launch_bounds__(kBlock)
sample_cdf_block_kernel(const uint64_t* __restrict__ off,
                        const float* __restrict__ w,
                        const uint32_t* __restrict__ rows, uint64_t nrows,
                        float* __restrict__ cdf) {
  __shared__ float s_wave[kBlock / kWave];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    const uint64_t b = off[r], e = off[r + 1];
    float carry = 0.f;
    for (uint64_t base = b; base < e; base += kBlock) {
      uint64_t idx = base + threadIdx.x;
      float s = wave_incl_scan_f32(idx < e ? w[idx] : 0.f);
      if (lane == 63) s_wave[wid] = s;
      __syncthreads();
      float before = 0.f, total = 0.f;
#pragma unroll
      for (uint32_t q = 0; q < kBlock / kWave; ++q) {
        if (q < wid) before += s_wave[q];
        total += s_wave[q];
      }
      if (idx < e) cdf[idx] = carry + (before + s);
      carry += total;
      __syncthreads();
    }
  }
}

// --- top-k index: k arg-max passes under (weight, -slot), three tiers -------

// larger key = earlier in the order: weight descending (-0 counts as +0),
// then the smaller slot. Keys of one row are distinct.
__device__ __forceinline__ uint64_t sample_key(float w, uint32_t slot) {
  uint32_t b = __float_as_uint(w + 0.f);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (static_cast<uint64_t>(b) << 32) | (0xFFFFFFFFu - slot);
}

__device__ __forceinline__ uint32_t sample_key_slot(uint64_t key) {
  return 0xFFFFFFFFu - static_cast<uint32_t>(key);
}

__global__ void sample_long_rows_kernel(const uint64_t* __restrict__ off,
                                        uint32_t rows_n, uint32_t k,
                                        uint32_t* __restrict__ flag) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows_n;
       r += stride)
    flag[r] = off[r + 1] - off[r] > k ? 1u : 0u;
}

__global__ void sample_topk_thread_kernel(
    const uint64_t* __restrict__ off, const float* __restrict__ w,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t k,
    const uint64_t* __restrict__ rank, uint32_t* __restrict__ slots) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < nrows; i += stride) {
    uint32_t r = rows[i];
    const uint64_t b = off[r];
    const uint32_t deg = static_cast<uint32_t>(off[r + 1] - b);
    uint32_t* out = slots + rank[r] * k;
    uint64_t prev = ~0ull;
    for (uint32_t p = 0; p < k; ++p) {
      uint64_t best = 0;
      for (uint32_t j = 0; j < deg; ++j) {
        uint64_t key = sample_key(w[b + j], j);
        if (key < prev && key > best) best = key;
      }
      out[p] = sample_key_slot(best);
      prev = best;
    }
  }
}

// a wave keeps the keys of its row (at most kSampleWaveDeg) in registers
__global__ void sample_topk_wave_kernel(
    const uint64_t* __restrict__ off, const float* __restrict__ w,
    const uint32_t* __restrict__ rows, uint64_t nrows, uint32_t k,
    const uint64_t* __restrict__ rank, uint32_t* __restrict__ slots) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nwaves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
  for (uint64_t i = (static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                     threadIdx.x) >> 6;
       i < nrows; i += nwaves) {
    uint32_t r = rows[i];
    const uint64_t b = off[r];
    const uint32_t deg = static_cast<uint32_t>(off[r + 1] - b);
    uint64_t key[kSampleWaveKeys];
#pragma unroll
    for (int j = 0; j < kSampleWaveKeys; ++j) {
      uint32_t slot = j * kWave + lane;
      key[j] = slot < deg ? sample_key(w[b + slot], slot) : 0;
    }
    uint32_t* out = slots + rank[r] * k;
    uint64_t prev = ~0ull;
    for (uint32_t p = 0; p < k; ++p) {
      uint64_t best = 0;
#pragma unroll
      for (int j = 0; j < kSampleWaveKeys; ++j)
        if (key[j] < prev && key[j] > best) best = key[j];
      best = wave_max_u64(best);
      if (lane == 0) out[p] = sample_key_slot(best);
      prev = best;
    }
  }
}

__global__ void __launch_bounds__(kBlock)
sample_topk_block_kernel(const uint64_t* __restrict__ off,
                         const float* __restrict__ w,
                         const uint32_t* __restrict__ rows, uint64_t nrows,
                         uint32_t k, const uint64_t* __restrict__ rank,
                         uint32_t* __restrict__ slots) {
  __shared__ uint64_t s_wave[kBlock / kWave];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (uint64_t i = blockIdx.x; i < nrows; i += gridDim.x) {
    uint32_t r = rows[i];
    const uint64_t b = off[r];
    const uint64_t deg = off[r + 1] - b;
    uint32_t* out = slots + rank[r] * k;
    uint64_t prev = ~0ull;
    for (uint32_t p = 0; p < k; ++p) {
      uint64_t best = 0;
      for (uint64_t j = threadIdx.x; j < deg; j += kBlock) {
        uint64_t key = sample_key(w[b + j], static_cast<uint32_t>(j));
        if (key < prev && key > best) best = key;
      }
      best = wave_max_u64(best);
      if (lane == 0) s_wave[wid] = best;
      __syncthreads();
#pragma unroll
      for (uint32_t q = 0; q < kBlock / kWave; ++q)
        if (s_wave[q] > best) best = s_wave[q];
      if (threadIdx.x == 0) out[p] = sample_key_slot(best);
      prev = best;
      __syncthreads();
    }
  }
}

// --- walker queues ----------------------------------------------------------

// cnt[0]: walkers in `next`, cnt[1]: steps taken, cnt[2 + p]: walkers in
// peer p's send region (cap entries each)
struct SampleQueues {
  SampleWalker* next;
  SampleWalker* peer;
  unsigned long long* cnt;
  uint64_t cap;
  int rank;
};

// Wave-aggregated append of one walker per lane to the queue of its target
// rank (target < 0: none): one atomic per wave and distinct target. Every
// lane of the wave calls it.
__device__ __forceinline__ void sample_append(const SampleQueues& q,
                                              int target, SampleWalker wk) {
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long remaining = __ballot(target >= 0);
  while (remaining) {
    const int L = __ffsll(remaining) - 1;
    const int t0 = __shfl(target, L, 64);
    const unsigned long long m = __ballot(target == t0) & remaining;
    remaining &= ~m;
    unsigned long long base = 0;
    if (lane == static_cast<uint32_t>(L))
      base = atomicAdd(t0 == q.rank ? q.cnt : q.cnt + 2 + t0,
                       static_cast<unsigned long long>(__popcll(m)));
    base = __shfl(base, L, 64);
    if (target == t0) {
      uint64_t at = base + __popcll(m & ((1ull << lane) - 1));
      SampleWalker* dst =
          t0 == q.rank ? q.next : q.peer + static_cast<uint64_t>(t0) * q.cap;
      if (at < q.cap) dst[at] = wk;
    }
  }
}

// Walk i starts on starts[i] (through perm on a hub-renumbered graph); the
// owner of that vertex writes paths[i][0] and queues the walker.
__global__ void sample_seed_kernel(const uint32_t* __restrict__ starts,
                                   uint64_t n_walks,
                                   const uint32_t* __restrict__ perm,
                                   uint32_t nv_global, uint32_t v_begin,
                                   uint32_t v_end,
                                   uint32_t* __restrict__ paths,
                                   uint32_t row_len, bool more,
                                   SampleQueues q) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                       (threadIdx.x - lane);
       base < n_walks; base += stride) {
    const uint64_t i = base + lane;
    int target = -1;
    SampleWalker wk{0, 0};
    if (i < n_walks) {
      uint32_t v = starts[i];
      if (v < nv_global) {
        if (perm) v = perm[v];
        if (v >= v_begin && v < v_end) {
          paths[i * row_len] = v;
          if (more) {
            target = q.rank;
            wk = SampleWalker{v, static_cast<uint32_t>(i)};
          }
        }
      }
    }
    sample_append(q, target, wk);
  }
}

struct SampleIndex {
  const float* __restrict__ cdf;          // edge_weight
  const uint64_t* __restrict__ topk_rank;  // top_k on a weighted graph,
  const uint32_t* __restrict__ topk_slots;  //   null otherwise
  uint32_t k;
};

enum { kSampleRandom = 0, kSampleEdgeWeight = 1, kSampleTopK = 2 };

// The slot that draw r takes out of the stored row `row` = arcs
// [b, b + deg), deg >= 1; deg itself at a dead end. The one pick rule of the
// walk step and of the fan-out level kernel.
template <int STRAT>
__device__ __forceinline__ uint64_t sample_pick(const SampleIndex& ix,
                                                uint32_t row, uint64_t b,
                                                uint64_t deg, uint64_t r) {
  uint64_t pick = deg;
  if constexpr (STRAT == kSampleRandom) {
    pick = __umul64hi(r, deg);
  } else if constexpr (STRAT == kSampleEdgeWeight) {
    const float* __restrict__ c = ix.cdf + b;
    const float total = c[deg - 1];
    if (total > 0.f) {
      const float u =
          static_cast<float>(static_cast<uint32_t>(r >> 40)) * 0x1p-24f;
      const float t = __fmul_rn(u, total);
      uint64_t lo = 0, hi = deg;
      while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        if (c[mid] <= t)
          lo = mid + 1;
        else
          hi = mid;
      }
      pick = lo < deg ? lo : deg - 1;
    }
  } else {
    const uint64_t kk = deg < ix.k ? deg : ix.k;
    pick = __umul64hi(r, kk);
    if (ix.topk_slots && deg > ix.k)
      pick = ix.topk_slots[ix.topk_rank[row] * ix.k + pick];
  }
  return pick;
}

// One lane per live walker of `cur`; `more`: hops remain after this one.
template <int STRAT>
__global__ void sample_step_kernel(DevGraphView g,
                                   const SampleWalker* __restrict__ cur,
                                   uint64_t n, SampleIndex ix,
                                   uint32_t* __restrict__ paths,
                                   uint32_t row_len, uint32_t hop, bool more,
                                   uint64_t seed, SampleQueues q) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                       (threadIdx.x - lane);
       base < n; base += stride) {
    const uint64_t i = base + lane;
    int target = -1;
    SampleWalker out{0, 0};
    bool stepped = false;
    if (i < n) {
      const SampleWalker wk = cur[i];
      const bool here = g.is_owned(wk.v);  // always: the sender checked
      const uint32_t row = here ? g.row(wk.v) : 0;
      const uint64_t b = g.oe_off[row];
      const uint64_t deg = here ? g.oe_off[row + 1] - b : 0;
      if (deg) {
        const uint64_t r = sample_draw(seed, wk.walk, hop);
        const uint64_t pick =
            sample_pick<STRAT>(ix, row, b, deg, r);  // deg: dead end
        if (pick < deg) {
          const uint32_t nv = g.oe_dst[b + pick];
          paths[static_cast<uint64_t>(wk.walk) * row_len + hop + 1] = nv;
          stepped = true;
          if (more) {
            target = g.owner(nv);
            out = SampleWalker{nv, wk.walk};
          }
        }
      }
    }
    const unsigned long long sm = __ballot(stepped);
    if (lane == 0 && sm)
      atomicAdd(q.cnt + 1, static_cast<unsigned long long>(__popcll(sm)));
    sample_append(q, target, out);
  }
}

// the rows of the owned walks out of the path table, hub renumbering undone
__global__ void sample_gather_kernel(const uint32_t* __restrict__ paths,
                                     const uint32_t* __restrict__ own,
                                     uint64_t n_own, uint32_t row_len,
                                     const uint32_t* __restrict__ inv,
                                     uint32_t* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const uint64_t total = n_own * row_len;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < total; i += stride) {
    uint32_t x = paths[static_cast<uint64_t>(own[i / row_len]) * row_len +
                       i % row_len];
    if (inv && x != kSampleNoVertex) x = inv[x];
    out[i] = x;
  }
}

// --- fan-out (neighbourhood) sampling ---------------------------------------
//
// Reference parity: examples/gnn_sampler --hop_and_num f_1-...-f_H: f_1
// neighbours of every seed, f_2 of each of those, ..., with replacement. The
// tree of seed i is level-major on the device: level h is one array of
// n * L_h ids (L_0 = 1, L_h = L_{h-1} * f_h), entry i * L_h + j being slot
// base_h + j of seed i (base_h = L_1 + ... + L_{h-1}). Item t of level h has
// its parent at t / f_h of level h - 1 and writes entry t: the f_h lanes of
// one parent are adjacent, read one parent entry and one pair of row offsets,
// and the child writes are coalesced. No queue, no append. The draw of item t
// is sample_draw(seed, t / L_h, base_h + t % L_h), the pick sample_pick.
// Every array is prefilled with kSampleNoVertex, so a dead parent leaves its
// subtree dead, and the owner of the parent's vertex alone writes: an
// element-wise min over ranks completes a level.

// a / d; `small`: both fit in 32 bits (one hardware-assisted divide)
__device__ __forceinline__ uint64_t fanout_div(uint64_t a, uint64_t d,
                                               bool small) {
  return small ? static_cast<uint32_t>(a) / static_cast<uint32_t>(d) : a / d;
}

// level 0: the seeds in stored ids, on every rank alike
__global__ void fanout_seed_kernel(const uint32_t* __restrict__ seeds,
                                   uint64_t n,
                                   const uint32_t* __restrict__ perm,
                                   uint32_t nv_global,
                                   uint32_t* __restrict__ level0) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < n; i += stride) {
    uint32_t v = seeds[i];
    if (v < nv_global) {
      if (perm) v = perm[v];
    } else {
      v = kSampleNoVertex;
    }
    level0[i] = v;
  }
}

// One lane per item of a level of n_items = n * L entries, fan-out f over
// `parents` (the level before, n_items / f entries); cnt: the draws made.
template <int STRAT>
__global__ void fanout_level_kernel(DevGraphView g,
                                    const uint32_t* __restrict__ parents,
                                    uint32_t* __restrict__ level,
                                    uint64_t n_items, uint32_t f, uint64_t L,
                                    uint64_t base_pos, SampleIndex ix,
                                    uint64_t seed,
                                    unsigned long long* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  const bool small = n_items <= 0xFFFFFFFFull;  // L and f are no larger
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                       (threadIdx.x - lane);
       base < n_items; base += stride) {
    const uint64_t t = base + lane;
    bool drew = false;
    if (t < n_items) {
      const uint32_t pv = parents[fanout_div(t, f, small)];
      if (pv != kSampleNoVertex && g.is_owned(pv)) {
        const uint32_t row = g.row(pv);
        const uint64_t b = g.oe_off[row];
        const uint64_t deg = g.oe_off[row + 1] - b;
        if (deg) {
          const uint64_t i = fanout_div(t, L, small);
          const uint64_t r = sample_draw(seed, i, base_pos + (t - i * L));
          const uint64_t pick = sample_pick<STRAT>(ix, row, b, deg, r);
          if (pick < deg) {
            level[t] = g.oe_dst[b + pick];
            drew = true;
          }
        }
      }
    }
    const unsigned long long dm = __ballot(drew);
    if (lane == 0 && dm)
      atomicAdd(cnt, static_cast<unsigned long long>(__popcll(dm)));
  }
}

// Without replacement (core/fanout.hpp has the rule): one group of W lanes
// per parent, W = 1 << log_w the smallest power of two >= f <= 64, lane c of
// the group its child c, 64 / W parents per wave. A parent's domain is its m
// arc slots (random: the row, top_k: the min(deg, k) heaviest). m <= f: child
// c < m is domain element c. m > f: Floyd's subset sampling in child order,
// step s broadcasting t_s = index(r_s, m - f + s + 1) from lane s to the
// group and lane s taking m - f + s where a lane below holds t_s already.
// Every lane of the wave runs all f steps, whatever its group is, so the
// shuffles and ballots are wave-wide; dead, foreign, short and tail groups
// only vote false.
template <int STRAT>
__global__ void fanout_level_norep_kernel(
    DevGraphView g, const uint32_t* __restrict__ parents,
    uint32_t* __restrict__ level, uint64_t n_items, uint32_t f,
    uint32_t log_w, uint64_t L, uint64_t base_pos, SampleIndex ix,
    uint64_t seed, unsigned long long* __restrict__ cnt) {
  static_assert(STRAT == kSampleRandom || STRAT == kSampleTopK,
                "no cdf rule without replacement");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = 1u << log_w;
  const uint32_t c = lane & (w - 1);   // child of the group's parent
  const uint32_t first = lane - c;     // the group's lane 0
  const unsigned long long gmask =
      (w == 64 ? ~0ull : (1ull << w) - 1) << first;
  const bool small = n_items <= 0xFFFFFFFFull;  // L and f are no larger
  const uint64_t n_par = fanout_div(n_items, f, small);
  const uint64_t Lp = fanout_div(L, f, small);  // parents per seed
  const uint64_t stride =
      (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> log_w;
  for (uint64_t base = (static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                        (threadIdx.x - lane)) >> log_w;
       base < n_par; base += stride) {
    const uint64_t p = base + (lane >> log_w);
    uint32_t row = 0;
    uint64_t b = 0, deg = 0, m = 0, t = 0;
    if (p < n_par) {
      const uint32_t pv = parents[p];
      if (pv != kSampleNoVertex && g.is_owned(pv)) {
        row = g.row(pv);
        b = g.oe_off[row];
        deg = g.oe_off[row + 1] - b;
        m = deg;
        if constexpr (STRAT == kSampleTopK) m = deg < ix.k ? deg : ix.k;
      }
    }
    const bool floyd = m > f;  // the same in every lane of a group
    if (floyd && c < f) {
      const uint64_t i = fanout_div(p, Lp, small);
      const uint64_t r =
          sample_draw(seed, i, base_pos + (p - i * Lp) * f + c);
      t = __umul64hi(r, m - f + c + 1);
    }
    uint64_t e = c;  // m <= f: domain element c
    for (uint32_t s = 0; s < f; ++s) {
      const uint64_t ts = __shfl(static_cast<unsigned long long>(t),
                                 static_cast<int>(first + s), 64);
      const unsigned long long taken =
          __ballot(floyd && c < s && e == ts) & gmask;
      if (floyd && c == s) e = taken ? m - f + s : ts;
    }
    const bool drew = c < f && (floyd || c < m);
    if (drew) {
      uint64_t slot = e;
      if constexpr (STRAT == kSampleTopK) {
        if (ix.topk_slots && deg > ix.k)
          slot = ix.topk_slots[ix.topk_rank[row] * ix.k + slot];
      }
      level[p * f + c] = g.oe_dst[b + slot];
    }
    const unsigned long long dm = __ballot(drew);
    if (lane == 0 && dm)
      atomicAdd(cnt, static_cast<unsigned long long>(__popcll(dm)));
  }
}

// level-major to root-major: columns [col0, col0 + L) of the rows of the
// owned seeds, hub renumbering undone
__global__ void fanout_gather_kernel(const uint32_t* __restrict__ level,
                                     const uint32_t* __restrict__ own,
                                     uint64_t n_own, uint64_t L,
                                     uint64_t row_len, uint64_t col0,
                                     const uint32_t* __restrict__ inv,
                                     uint32_t* __restrict__ out) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const uint64_t total = n_own * L;
  const bool small = total <= 0xFFFFFFFFull;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x +
                    threadIdx.x;
       i < total; i += stride) {
    const uint64_t r = fanout_div(i, L, small);
    const uint64_t j = i - r * L;
    uint32_t x = level[static_cast<uint64_t>(own[r]) * L + j];
    if (inv && x != kSampleNoVertex) x = inv[x];
    out[r * row_len + col0 + j] = x;
  }
}

namespace {

void ensure_sample_cdf(DeviceGraph& g, GpuContext::Impl& I, hipStream_t s) {
  if (g.sample_cdf_built) return;
  HIP_CHECK(hipStreamSynchronize(s));
  const double t0 = wall_s();
  const uint32_t owned = g.owned();
  const uint64_t arcs = g.oe_dst.size();
  g.sample_cdf.resize(arcs ? arcs : 1);
  if (owned && arcs) {
    DeviceBuffer<uint32_t> rt, rw, rb;
    auto n = partition_rows(SampleLenTiers{g.oe_off.data(), 0}, owned,
                            {&rt, &rw, &rb}, s);
    const uint64_t* off = g.oe_off.data();
    const float* w = g.oe_w.data();
    float* cdf = g.sample_cdf.data();
    if (n[2])
      sample_cdf_block_kernel<<<std::min<uint64_t>(n[2], kMaxGrid), kBlock, 0,
                                s>>>(off, w, rb.data(), n[2], cdf);
    if (n[1])
      sample_cdf_wave_kernel<<<grid_for(n[1] * kWave), kBlock, 0, s>>>(
          off, w, rw.data(), n[1], cdf);
    if (n[0])
      sample_cdf_thread_kernel<<<grid_for(n[0]), kBlock, 0, s>>>(
          off, w, rt.data(), n[0], cdf);
    HIP_CHECK(hipStreamSynchronize(s));  // the row lists go out of scope
  }
  g.sample_cdf_built = true;
  ++I.sample_dbg.cdf_builds;
  I.sample_dbg.cdf_bytes = g.sample_cdf.size() * sizeof(float);
  I.sample_dbg.cdf_ms = (wall_s() - t0) * 1e3;
}

void ensure_sample_topk(DeviceGraph& g, GpuContext::Impl& I, int k,
                        hipStream_t s) {
  if (g.sample_topk_k == k) return;
  HIP_CHECK(hipStreamSynchronize(s));
  const double t0 = wall_s();
  const uint32_t owned = g.owned();
  const uint32_t uk = static_cast<uint32_t>(k);
  g.sample_topk_k = 0;
  g.sample_topk_rank.resize(static_cast<size_t>(owned) + 1);
  uint64_t n_long = 0;
  {
    DeviceBuffer<uint32_t> flag(owned ? owned : 1);
    if (owned)
      sample_long_rows_kernel<<<grid_for(owned), kBlock, 0, s>>>(
          g.oe_off.data(), owned, uk, flag.data());
    n_long = exclusive_scan(flag.data(), g.sample_topk_rank.data(), owned, s,
                            I.scan);
  }
  g.sample_topk_slots.resize(n_long ? n_long * uk : 1);
  if (n_long) {
    DeviceBuffer<uint32_t> rt, rw, rb;
    auto n = partition_rows(SampleLenTiers{g.oe_off.data(), uk}, owned,
                            {&rt, &rw, &rb}, s);
    const uint64_t* off = g.oe_off.data();
    const float* w = g.oe_w.data();
    const uint64_t* rank = g.sample_topk_rank.data();
    uint32_t* slots = g.sample_topk_slots.data();
    if (n[2])
      sample_topk_block_kernel<<<std::min<uint64_t>(n[2], kMaxGrid), kBlock,
                                 0, s>>>(off, w, rb.data(), n[2], uk, rank,
                                         slots);
    if (n[1])
      sample_topk_wave_kernel<<<grid_for(n[1] * kWave), kBlock, 0, s>>>(
          off, w, rw.data(), n[1], uk, rank, slots);
    if (n[0])
      sample_topk_thread_kernel<<<grid_for(n[0]), kBlock, 0, s>>>(
          off, w, rt.data(), n[0], uk, rank, slots);
    HIP_CHECK(hipStreamSynchronize(s));  // the row lists go out of scope
  }
  g.sample_topk_k = k;
  ++I.sample_dbg.topk_builds;
  I.sample_dbg.topk_bytes = g.sample_topk_rank.size() * sizeof(uint64_t) +
                            g.sample_topk_slots.size() * sizeof(uint32_t);
  I.sample_dbg.topk_ms = (wall_s() - t0) * 1e3;
}

template <int STRAT>
void launch_sample_step(hipStream_t s, const DevGraphView& view,
                        const SampleWalker* cur, uint64_t n,
                        const SampleIndex& ix, uint32_t* paths,
                        uint32_t row_len, uint32_t hop, bool more,
                        uint64_t seed, const SampleQueues& q) {
  sample_step_kernel<STRAT><<<grid_for(n), kBlock, 0, s>>>(
      view, cur, n, ix, paths, row_len, hop, more, seed, q);
}

}  // namespace

GpuRunResult GpuContext::sample(DeviceGraph& g,
                                const std::vector<uint32_t>& starts,
                                int hops, int strategy, int top_k,
                                uint64_t seed) {
  RangeMarker _mk("grapehip::sample");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  if (strategy < kSampleRandom || strategy > kSampleTopK)
    throw std::runtime_error("sample: strategy must be 0, 1 or 2");
  if (hops < 0) throw std::runtime_error("sample: hops must be >= 0");
  if (strategy == kSampleTopK && (top_k < 1 || top_k > kSampleTopKMax))
    throw std::runtime_error("sample: top_k = " + std::to_string(top_k) +
                             " is outside 1.." +
                             std::to_string(kSampleTopKMax) +
                             " (kSampleTopKMax) of the device sampler");
  const uint64_t n_walks = starts.size();
  const uint32_t row_len = static_cast<uint32_t>(hops) + 1;
  if (n_walks >= 0xFFFFFFFFull)
    throw std::runtime_error("sample: the walk index must fit in 32 bits");
  const bool multi = world_ > 1;
  // every weight of an unweighted graph is 1
  if (strategy == kSampleEdgeWeight && !g.weighted) strategy = kSampleRandom;
  SampleIndex ix{nullptr, nullptr, nullptr, static_cast<uint32_t>(top_k)};
  if (strategy == kSampleEdgeWeight) {
    ensure_sample_cdf(g, I, s);
    ix.cdf = g.sample_cdf.data();
  } else if (strategy == kSampleTopK && g.weighted) {
    ensure_sample_topk(g, I, top_k, s);
    ix.topk_rank = g.sample_topk_rank.data();
    ix.topk_slots = g.sample_topk_slots.data();
  }

  // the walks that start here, by the ids as loaded: the hub renumbering
  // permutes inside a slice, so it keeps the owner
  std::vector<uint32_t> own;
  for (uint64_t i = 0; i < n_walks; ++i)
    if (starts[i] < g.nv_global && starts[i] >= g.v_begin &&
        starts[i] < g.v_end)
      own.push_back(static_cast<uint32_t>(i));

  const uint64_t cap = n_walks ? n_walks : 1;
  grow(I.sample_q[0], cap);
  grow(I.sample_q[1], cap);
  if (multi) grow(I.sample_peer, cap * world_);
  grow(I.sample_cnt, static_cast<size_t>(world_) + 2);
  grow(I.sample_paths, cap * row_len);
  grow(I.sample_starts, cap);
  grow(I.sample_own, own.size() ? own.size() : 1);
  grow(I.sample_out, own.size() ? own.size() * row_len : 1);
  const size_t n_cnt = static_cast<size_t>(world_) + 2;
  DevGraphView view = make_view(g, rank_, world_);

  RunBracket br(I, comm_);

  if (n_walks)
    HIP_CHECK(hipMemcpyAsync(I.sample_starts.data(), starts.data(),
                             n_walks * 4, hipMemcpyHostToDevice, s));
  fill(I.sample_paths.data(), kSampleNoVertex, n_walks * row_len, s);
  HIP_CHECK(hipMemsetAsync(I.sample_cnt.data(), 0, n_cnt * 8, s));
  int cur = 0;
  auto queues = [&](int next) {
    return SampleQueues{
        reinterpret_cast<SampleWalker*>(I.sample_q[next].data()),
        reinterpret_cast<SampleWalker*>(I.sample_peer.data()),
        I.sample_cnt.data(), cap, rank_};
  };
  if (n_walks)
    sample_seed_kernel<<<grid_for(n_walks), kBlock, 0, s>>>(
        I.sample_starts.data(), n_walks,
        g.permuted ? g.perm.data() : nullptr, g.nv_global, g.v_begin,
        g.v_end, I.sample_paths.data(), row_len, hops > 0, queues(cur));
  std::vector<unsigned long long> c(n_cnt);
  HIP_CHECK(hipMemcpyAsync(c.data(), I.sample_cnt.data(), n_cnt * 8,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  uint64_t n_cur = c[0];
  uint64_t live = multi ? comm_->allreduce_sum(n_cur) : n_cur;
  uint64_t steps = 0;
  int rounds = 0;
  for (int hop = 0; hop < hops && live; ++hop) {
    ++rounds;
    const bool more = hop + 1 < hops;
    const int nxt = cur ^ 1;
    HIP_CHECK(hipMemsetAsync(I.sample_cnt.data(), 0, n_cnt * 8, s));
    if (n_cur) {
      auto launch = strategy == kSampleRandom
                        ? launch_sample_step<kSampleRandom>
                        : (strategy == kSampleEdgeWeight
                               ? launch_sample_step<kSampleEdgeWeight>
                               : launch_sample_step<kSampleTopK>);
      launch(s, view,
             reinterpret_cast<const SampleWalker*>(I.sample_q[cur].data()),
             n_cur, ix, I.sample_paths.data(), row_len,
             static_cast<uint32_t>(hop), more, seed, queues(nxt));
    }
    // the one count read per round
    HIP_CHECK(hipMemcpyAsync(c.data(), I.sample_cnt.data(), n_cnt * 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    steps += c[1];
    uint64_t n_next = c[0];
    live = n_next;
    if (multi && more) {
      // lengths on the control plane: [p] walkers for peer p, [world] the
      // walkers that stay
      std::vector<uint64_t> mine(world_ + 1), all(
          static_cast<size_t>(world_) * (world_ + 1));
      for (int p = 0; p < world_; ++p) mine[p] = p == rank_ ? 0 : c[2 + p];
      mine[world_] = n_next;
      comm_->allgather(mine.data(), mine.size() * 8, all.data());
      std::vector<uint64_t> send_off(world_ + 1, 0), recv_off(world_ + 1, 0);
      live = 0;
      for (int p = 0; p < world_; ++p) {
        const uint64_t* row = all.data() + static_cast<size_t>(p) *
                                               (world_ + 1);
        send_off[p + 1] = send_off[p] + mine[p] * sizeof(SampleWalker);
        recv_off[p + 1] = recv_off[p] + row[rank_] * sizeof(SampleWalker);
        for (int t = 0; t <= world_; ++t) live += row[t];
      }
      const uint64_t n_recv = recv_off[world_] / sizeof(SampleWalker);
      if (n_next + n_recv > cap)
        throw std::runtime_error("sample: more walkers than walks");
      // regions packed in peer order; the payload lands behind the walkers
      // that stayed
      if (I.sendbuf.size() < send_off[world_])
        I.sendbuf.resize(send_off[world_] + (1 << 20));
      for (int p = 0; p < world_; ++p)
        if (mine[p])
          HIP_CHECK(hipMemcpyAsync(
              I.sendbuf.data() + send_off[p],
              I.sample_peer.data() + static_cast<uint64_t>(p) * cap,
              mine[p] * sizeof(SampleWalker), hipMemcpyDeviceToDevice, s));
      I.dc.sendrecv(I.sendbuf.data(), send_off,
                    reinterpret_cast<uint8_t*>(I.sample_q[nxt].data() +
                                               n_next),
                    recv_off, s);
      n_next += n_recv;
    }
    n_cur = n_next;
    cur = nxt;
  }
  // each slot was written by at most one rank over 0xFFFFFFFF
  if (multi && n_walks)
    I.dc.allreduce_min_u32(I.sample_paths.data(), n_walks * row_len, s);
  std::vector<uint32_t> paths_h;
  if (!own.empty()) {
    HIP_CHECK(hipMemcpyAsync(I.sample_own.data(), own.data(), own.size() * 4,
                             hipMemcpyHostToDevice, s));
    sample_gather_kernel<<<grid_for(own.size() * row_len), kBlock, 0, s>>>(
        I.sample_paths.data(), I.sample_own.data(), own.size(), row_len,
        g.permuted ? g.inv.data() : nullptr, I.sample_out.data());
    paths_h.resize(own.size() * row_len);
    HIP_CHECK(hipMemcpyAsync(paths_h.data(), I.sample_out.data(),
                             paths_h.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  if (multi) steps = comm_->allreduce_sum(steps);
  ++I.sample_dbg.calls;
  I.sample_dbg.steps = steps;
  GpuRunResult res = br.finish(rounds, steps);
  res.paths = std::move(paths_h);
  res.walk_ids.assign(own.begin(), own.end());
  return res;
}

namespace {

template <int STRAT>
void launch_fanout_level(hipStream_t s, const DevGraphView& view,
                         const uint32_t* parents, uint32_t* level,
                         uint64_t n_items, uint32_t f, uint64_t L,
                         uint64_t base_pos, const SampleIndex& ix,
                         uint64_t seed, unsigned long long* cnt) {
  fanout_level_kernel<STRAT><<<grid_for(n_items), kBlock, 0, s>>>(
      view, parents, level, n_items, f, L, base_pos, ix, seed, cnt);
}

// one group of the smallest power of two >= f lanes per parent
template <int STRAT>
void launch_fanout_level_norep(hipStream_t s, const DevGraphView& view,
                               const uint32_t* parents, uint32_t* level,
                               uint64_t n_items, uint32_t f, uint64_t L,
                               uint64_t base_pos, const SampleIndex& ix,
                               uint64_t seed, unsigned long long* cnt) {
  uint32_t log_w = 0;
  while ((1u << log_w) < f) ++log_w;  // f <= kFanoutNoReplaceMax = 64
  fanout_level_norep_kernel<STRAT>
      <<<grid_for((n_items / f) << log_w), kBlock, 0, s>>>(
          view, parents, level, n_items, f, log_w, L, base_pos, ix, seed,
          cnt);
}

}  // namespace

GpuRunResult GpuContext::sample_neighbors(DeviceGraph& g,
                                          const std::vector<uint32_t>& seeds,
                                          const std::vector<int64_t>& fanouts,
                                          int strategy, int top_k,
                                          uint64_t seed, bool replace) {
  RangeMarker _mk("grapehip::sample_neighbors");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  if (strategy < kSampleRandom || strategy > kSampleTopK)
    throw std::runtime_error("sample_neighbors: strategy must be 0, 1 or 2");
  if (strategy == kSampleTopK && (top_k < 1 || top_k > kSampleTopKMax))
    throw std::runtime_error("sample_neighbors: top_k = " +
                             std::to_string(top_k) + " is outside 1.." +
                             std::to_string(kSampleTopKMax) +
                             " (kSampleTopKMax) of the device sampler");
  const uint64_t n = seeds.size();
  // sizes checked in 64 bits before anything is allocated
  const FanoutLayout lay = fanout_layout(fanouts, n);
  const int H = lay.levels();
  const uint64_t row_len = lay.row_len();
  const bool multi = world_ > 1;
  // every weight of an unweighted graph is 1
  if (strategy == kSampleEdgeWeight && !g.weighted) strategy = kSampleRandom;
  if (!replace) {
    fanout_check_no_replace(strategy == kSampleEdgeWeight);
    // one wave holds the picks of a parent
    for (uint64_t f : lay.fan)
      if (f > kFanoutNoReplaceMax)
        throw std::runtime_error(
            "sample_neighbors: fanout = " + std::to_string(f) +
            " is above " + std::to_string(kFanoutNoReplaceMax) +
            " (kFanoutNoReplaceMax) of the device sampler with "
            "replace=False");
  }
  SampleIndex ix{nullptr, nullptr, nullptr, static_cast<uint32_t>(top_k)};
  if (strategy == kSampleEdgeWeight) {
    ensure_sample_cdf(g, I, s);
    ix.cdf = g.sample_cdf.data();
  } else if (strategy == kSampleTopK && g.weighted) {
    ensure_sample_topk(g, I, top_k, s);
    ix.topk_rank = g.sample_topk_rank.data();
    ix.topk_slots = g.sample_topk_slots.data();
  }

  // the seeds owned here, by the ids as loaded (the hub renumbering keeps
  // the owner), and the live parents of level 1
  std::vector<uint32_t> own;
  uint64_t live = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (seeds[i] >= g.nv_global) continue;
    ++live;
    if (seeds[i] >= g.v_begin && seeds[i] < g.v_end)
      own.push_back(static_cast<uint32_t>(i));
  }

  // workspace shared with sample(): the levels lie one after the other in
  // sample_paths, level h at n * col[h]
  const uint64_t cap = n ? n : 1;
  const size_t n_cnt = static_cast<size_t>(H) + 1;
  grow(I.sample_paths, cap * row_len);
  grow(I.sample_starts, cap);
  grow(I.sample_cnt, n_cnt);
  grow(I.sample_own, own.size() ? own.size() : 1);
  grow(I.sample_out, own.size() ? own.size() * row_len : 1);
  DevGraphView view = make_view(g, rank_, world_);
  uint32_t* levels = I.sample_paths.data();

  RunBracket br(I, comm_);

  uint64_t draws = 0;
  int rounds = 0;
  if (n) {
    HIP_CHECK(hipMemcpyAsync(I.sample_starts.data(), seeds.data(), n * 4,
                             hipMemcpyHostToDevice, s));
    fill(levels, kSampleNoVertex, n * row_len, s);
    HIP_CHECK(hipMemsetAsync(I.sample_cnt.data(), 0, n_cnt * 8, s));
    fanout_seed_kernel<<<grid_for(n), kBlock, 0, s>>>(
        I.sample_starts.data(), n, g.permuted ? g.perm.data() : nullptr,
        g.nv_global, levels);
    auto launch = strategy == kSampleRandom
                      ? launch_fanout_level<kSampleRandom>
                      : (strategy == kSampleEdgeWeight
                             ? launch_fanout_level<kSampleEdgeWeight>
                             : launch_fanout_level<kSampleTopK>);
    if (!replace)
      launch = strategy == kSampleRandom
                   ? launch_fanout_level_norep<kSampleRandom>
                   : launch_fanout_level_norep<kSampleTopK>;
    for (int h = 1; h <= H && live; ++h) {
      ++rounds;
      const uint64_t L = lay.len[h];
      uint32_t* level = levels + n * lay.col[h];
      launch(s, view, levels + n * lay.col[h - 1], level, n * L,
             static_cast<uint32_t>(lay.fan[h - 1]), L, lay.col[h] - 1, ix,
             seed, I.sample_cnt.data() + h);
      // the one count read per level
      unsigned long long c = 0;
      HIP_CHECK(hipMemcpyAsync(&c, I.sample_cnt.data() + h, 8,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      live = multi ? comm_->allreduce_sum(static_cast<uint64_t>(c)) : c;
      draws += live;
      // each entry was written by at most one rank over 0xFFFFFFFF
      if (multi && live) I.dc.allreduce_min_u32(level, n * L, s);
    }
  }
  std::vector<uint32_t> rows_h;
  if (!own.empty()) {
    HIP_CHECK(hipMemcpyAsync(I.sample_own.data(), own.data(), own.size() * 4,
                             hipMemcpyHostToDevice, s));
    for (int h = 0; h <= H; ++h)
      fanout_gather_kernel<<<grid_for(own.size() * lay.len[h]), kBlock, 0,
                             s>>>(
          levels + n * lay.col[h], I.sample_own.data(), own.size(),
          lay.len[h], row_len, lay.col[h],
          g.permuted ? g.inv.data() : nullptr, I.sample_out.data());
    rows_h.resize(own.size() * row_len);
    HIP_CHECK(hipMemcpyAsync(rows_h.data(), I.sample_out.data(),
                             rows_h.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  ++I.sample_dbg.fanout_calls;
  I.sample_dbg.fanout_draws = draws;
  GpuRunResult res = br.finish(rounds, draws);
  res.paths = std::move(rows_h);
  res.walk_ids.assign(own.begin(), own.end());
  return res;
}

GpuContext::SampleDebug GpuContext::debug_sample(bool reset) {
  SampleDebug out = impl_->sample_dbg;
  if (reset)
    impl_->sample_dbg.calls = impl_->sample_dbg.cdf_builds =
        impl_->sample_dbg.topk_builds = impl_->sample_dbg.steps =
            impl_->sample_dbg.fanout_calls = impl_->sample_dbg.fanout_draws =
                0;
  return out;
}

}  // namespace grapehip

namespace grapehip {

// ---------------------------------------------------------------------------
// k-core / core decomposition (frontier peeling; kernels in the app-functor
// section above). Reference parity: examples/analytical_apps/kcore/kcore.h
// and core_decomposition/core_decomposition.h.
//
// Level k is the minimum residual degree over the unpeeled owned rows (min
// across ranks), so empty levels are jumped. Within a level, sub-rounds
// expand the frontier through expand_frontier (GRAPEHIP_LB applies) until no
// rank has a vertex left at or below k. kcore(k) is the single level k - 1.
// Multi-rank: decrements of remote vertices accumulate in dec[] (global
// size, zero between flushes) and travel as (v, count) halo pairs; frontier
// emptiness and the level are agreed on the TCP control plane.
// Only real rows (< owned_real) are seeded or reduced over: padding rows
// have no arcs, are never referenced, and are cut from the results.
// ---------------------------------------------------------------------------
GpuRunResult GpuContext::peel(DeviceGraph& g, bool all_levels, int k,
                              bool fetch) {
  auto& I = *impl_;
  hipStream_t s = I.compute;
  DevGraphView view = make_view(g, rank_, world_);
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  uint32_t rows = g.owned_real;
  uint64_t cap = view.slice;
  bool multi = world_ > 1;
  // a directed vertex can lose up to its in-degree below zero; in-degrees
  // are not stored, so bound them by the arc total
  if (g.directed && g.total_edges > static_cast<uint64_t>(INT_MAX))
    throw std::runtime_error(
        "kcore: directed graphs need fewer than 2^31 arcs on the device");

  DeviceBuffer<int> deg(owned ? owned : 1);
  DeviceBuffer<int> core(owned ? owned : 1);
  DeviceBuffer<int> scal(2);  // [0] min alive degree, [1] row-too-long flag
  DeviceBuffer<uint32_t> q(owned + 64);
  size_t bm_words = (static_cast<size_t>(owned) + 31) / 32 + 1;
  DeviceBuffer<uint32_t> next_bm(bm_words);
  DeviceBuffer<uint32_t> dec(multi ? nv_pad : 1);
  const DevHalo halo = halo_reserve(
      I, world_, cap, view.slice, (static_cast<uint64_t>(nv_pad) + 31) / 32);

  RunBracket br(I, comm_);

  int rounds = 0;
  core.fill_bytes(0xFF, s);  // -1: not peeled
  // k <= 0 keeps every vertex: nothing to peel
  const bool run = all_levels || k > 0;
  if (run) {
    next_bm.zero(s);
    scal.zero(s);
    if (multi) {
      dec.zero(s);
      halo_reset(I, s);
    }
    kcore_init_deg_kernel<<<grid_for(owned), kBlock, 0, s>>>(
        g.oe_off.data(), owned, deg.data(), scal.data() + 1);
    if (owned) {
      int nchunks = static_cast<int>((owned + kBlock - 1) / kBlock);
      expand_cm_range<false, KcoreSelfLoopOp>
          <<<std::min(nchunks, kMaxGrid), kBlock, 0, s>>>(
              view, KcoreSelfLoopOp{deg.data(), g.v_begin});
    }
    int too_long = 0;
    HIP_CHECK(hipMemcpyAsync(&too_long, scal.data() + 1, 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    // agreed across ranks so that nobody is left waiting in a collective
    if (multi) too_long = comm_->allreduce_or(too_long != 0) ? 1 : 0;
    if (too_long)
      throw std::runtime_error("kcore: a row has 2^31 arcs or more");
  }

  int level = run && !all_levels ? k - 1 : 0;
  while (run) {
    if (all_levels) {
      fill(scal.data(), INT_MAX, 1, s);
      kcore_min_alive_kernel<<<grid_for(rows), kBlock, 0, s>>>(
          deg.data(), core.data(), rows, scal.data());
      int lmin = INT_MAX;
      HIP_CHECK(hipMemcpyAsync(&lmin, scal.data(), 4, hipMemcpyDeviceToHost,
                               s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (multi) {
        std::vector<int> all(world_);
        comm_->allgather(&lmin, sizeof(int), all.data());
        lmin = *std::min_element(all.begin(), all.end());
      }
      if (lmin == INT_MAX) break;  // every vertex on every rank is peeled
      level = lmin;
    }
    kcore_seed_kernel<<<grid_for(rows), kBlock, 0, s>>>(
        deg.data(), core.data(), rows, level, next_bm.data());
    uint64_t global_curr = 0;
    uint32_t qn =
        compact_frontier_global(I, comm_, world_, next_bm.data(), owned,
                                g.v_begin, q.data(), s, global_curr);
    int level_rounds = 0;
    while (global_curr > 0) {
      if (qn) {
        kcore_stamp_kernel<<<grid_for(qn), kBlock, 0, s>>>(
            q.data(), qn, g.v_begin, level, core.data());
        expand_frontier(
            I, view, q.data(), qn,
            KcoreOp{deg.data(), level, DevBitmap{next_bm.data()}, g.v_begin,
                    g.v_end, multi, dec.data(), halo},
            s);
      }
      if (multi)
        halo_round<uint32_t, true>(
            I, comm_, rank_, world_, dec.data(), cap,
            KcoreRecvOp{deg.data(), level, DevBitmap{next_bm.data()},
                        g.v_begin},
            s);
      qn = compact_frontier_global(I, comm_, world_, next_bm.data(), owned,
                                   g.v_begin, q.data(), s, global_curr);
      ++level_rounds;
    }
    rounds += level_rounds;
    if (getenv("GRAPEHIP_DEBUG"))
      fprintf(stderr, "[kcore] level=%d subrounds=%d t=%.1fms\n", level,
              level_rounds, br.elapsed_ms());
    if (!all_levels) break;
  }
  GpuRunResult res = br.finish(rounds, g.input_edges);
  if (fetch) {
    std::vector<int> c32(owned);
    if (owned)
      HIP_CHECK(hipMemcpyAsync(c32.data(), core.data(), owned * 4ull,
                               hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    res.i64.resize(owned);
    for (uint32_t i = 0; i < owned; ++i)
      res.i64[i] = all_levels ? (c32[i] < 0 ? 0 : c32[i])
                              : (i < rows && c32[i] < 0 ? 1 : 0);
  }
  return res;
}

GpuRunResult GpuContext::kcore(DeviceGraph& g, int k, bool fetch) {
  RangeMarker _mk("grapehip::kcore");
  return peel(g, /*all_levels=*/false, k, fetch);
}

GpuRunResult GpuContext::core_decomposition(DeviceGraph& g, bool fetch) {
  RangeMarker _mk("grapehip::core_decomposition");
  return peel(g, /*all_levels=*/true, 0, fetch);
}

// ---------------------------------------------------------------------------
// Betweenness centrality, single source (functors in the app-functor section
// above). Reference parity: examples/analytical_apps/bc/staged_bc{,_bfs}.h
// through cpp/apps/bc.hpp.
//
// Forward: push-only level-synchronous BFS through launch_expand (GRAPEHIP_LB
// applies). Each level's frontier is compacted into the next slice of one
// owned-size order array; the slice offsets stay on the host. Backward: the
// slices are replayed deepest first, a finalise kernel and one
// expand_frontier per level, so a single rank reads nothing back.
// Multi-rank: contributions to remote vertices sit in the remote entries of
// sigma / acc and travel as (v, fp64) take-and-zero halo pairs, one flush per
// level in each direction; every rank runs every flush. After the forward
// pass the remote depth copies are upper bounds only (the level at which this
// rank first reached the vertex), so one mirror refresh brings the owners'
// depths before the backward test depth[u] == d - 1 reads them.
// ---------------------------------------------------------------------------
GpuRunResult GpuContext::bc(DeviceGraph& g, int64_t source, bool fetch) {
  RangeMarker _mk("grapehip::bc");
  static_assert(sizeof(HaloPair<double>) == 16,
                "fp64 halo pairs pack at a 16-byte stride");
  auto& I = *impl_;
  hipStream_t s = I.compute;
  DevGraphView view = make_view(g, rank_, world_);
  uint32_t nv_pad = padded_nv(g, world_);
  uint32_t owned = g.owned();
  uint64_t cap = view.slice;
  bool multi = world_ > 1;

  if (multi) ensure_mirrors(I, comm_, g, rank_, world_, s);

  size_t bm_words = (static_cast<size_t>(owned) + 31) / 32 + 1;
  grow(I.trav_state, nv_pad);
  grow(I.trav_q[0], static_cast<size_t>(owned) + 64);
  grow(I.trav_near_bm, bm_words);
  grow(I.bc_sigma, nv_pad);
  grow(I.bc_acc, nv_pad);
  grow(I.bc_coef, static_cast<size_t>(owned) + 1);
  uint32_t* const depth = I.trav_state.data();
  uint32_t* const order = I.trav_q[0].data();
  uint32_t* const next_bm = I.trav_near_bm.data();
  double* const sigma = I.bc_sigma.data();
  double* const acc = I.bc_acc.data();
  double* const coef = I.bc_coef.data();
  DeviceBuffer<uint32_t>& fdeg = I.trav_fdeg;
  DeviceBuffer<uint64_t>& foff = I.trav_foff;
  const DevHalo halo = halo_reserve(
      I, world_, cap, view.slice, (static_cast<uint64_t>(nv_pad) + 31) / 32);

  RunBracket br(I, comm_);

  if (nv_pad) {
    HIP_CHECK(hipMemsetAsync(depth, 0xFF, static_cast<size_t>(nv_pad) * 4, s));
    HIP_CHECK(hipMemsetAsync(sigma, 0, static_cast<size_t>(nv_pad) * 8, s));
    HIP_CHECK(hipMemsetAsync(acc, 0, static_cast<size_t>(nv_pad) * 8, s));
  }
  HIP_CHECK(hipMemsetAsync(next_bm, 0, bm_words * 4, s));
  if (multi) halo_reset(I, s);
  uint32_t src = map_source(g, source, s);
  if (src >= g.v_begin && src < g.v_end)
    bc_seed_kernel<<<1, 1, 0, s>>>(depth, sigma, src, g.v_begin, next_bm);

  // level_off[d] .. level_off[d + 1]: level d's slice of the order array.
  // Every owned vertex enters one frontier, so the slices fit in `owned`.
  std::vector<uint64_t> level_off{0};
  uint64_t global_curr = 0;
  uint32_t qn = compact_frontier_global(I, comm_, world_, next_bm, owned,
                                        g.v_begin, order, s, global_curr);
  uint32_t level = 0;
  while (global_curr > 0) {
    const uint32_t* q = order + level_off.back();
    level_off.push_back(level_off.back() + qn);
    uint64_t fedges = scan_frontier_degrees(I, view, q, qn, fdeg, foff, s);
    launch_expand(I, view, q, qn, foff.data(), fedges,
                  BcFwdOp{depth, sigma, level + 1, DevBitmap{next_bm},
                          g.v_begin, g.v_end, multi, halo},
                  s);
    if (multi)
      halo_round<double, true>(
          I, comm_, rank_, world_, sigma, cap,
          BcFwdRecvOp{depth, sigma, level + 1, DevBitmap{next_bm}, g.v_begin},
          s);
    qn = compact_frontier_global(I, comm_, world_, next_bm, owned, g.v_begin,
                                 order + level_off.back(), s, global_curr);
    if (getenv("GRAPEHIP_DEBUG"))
      fprintf(stderr, "[bc] fwd level=%u fedges=%lu next=%u t=%.1fms\n",
              level, (unsigned long)fedges, qn, br.elapsed_ms());
    ++level;
  }
  const int levels = static_cast<int>(level);

  if (multi && levels > 1) {
    mirror_sync_begin(I, g, depth, s);
    mirror_sync_end(I, g, depth, s);
  }
  for (int d = levels - 1; d >= 0; --d) {
    const uint32_t* q = order + level_off[d];
    const uint32_t n = static_cast<uint32_t>(level_off[d + 1] - level_off[d]);
    if (n)
      bc_finalize_kernel<<<grid_for(n), kBlock, 0, s>>>(q, n, g.v_begin,
                                                        sigma, acc, coef);
    if (d == 0) break;  // the source has nothing above it
    expand_frontier(I, view, q, n,
                    BcBackOp{depth, coef, acc, static_cast<uint32_t>(d - 1),
                             g.v_begin, g.v_end, multi, halo},
                    s);
    if (multi)
      halo_round<double, true>(I, comm_, rank_, world_, acc, cap,
                               BcBackRecvOp{acc}, s);
    if (getenv("GRAPEHIP_DEBUG"))
      fprintf(stderr, "[bc] back level=%d slice=%u t=%.1fms\n", d, n,
              br.elapsed_ms());
  }
  GpuRunResult res = br.finish(levels, g.input_edges);
  if (fetch) {
    res.f64.resize(owned);
    res.f64b.resize(owned);
    if (owned) {
      HIP_CHECK(hipMemcpyAsync(res.f64.data(), acc + g.v_begin, owned * 8ull,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(res.f64b.data(), sigma + g.v_begin,
                               owned * 8ull, hipMemcpyDeviceToHost, s));
    }
    res.i64 = fetch_depth_i64(depth, g, s);  // syncs s: all three landed
  }
  return res;
}

}  // namespace grapehip
