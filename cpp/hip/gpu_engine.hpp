// grapehip — GPU engine interface (host side).
//
// Reference parity: grape/cuda/worker/gpu_worker.h + gpu_message_manager.h
// reimagined: TCP control plane (lengths, termination, scalar collectives) +
// RCCL-over-xGMI data plane, dual HIP streams. One GpuContext per process ==
// one MI355X GPU == one fragment.
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <vector>

#include "../core/fanout.hpp"
#include "../core/fragment.hpp"
#include "../core/net.hpp"
#include "../core/types.hpp"
#include "dev_graph.hpp"
#include "hip_common.hpp"

struct ncclComm;  // fwd (rccl.h included in the .hip TU)

namespace grapehip {

struct DeviceGraph {
  uint32_t nv_global = 0;   // device id space (padded for dense renumber)
  uint64_t nv_real = 0;     // true vertex count (PageRank N etc.)
  uint32_t v_begin = 0, v_end = 0;
  uint32_t owned_real = 0;  // rows with real vertices (<= owned(); dense
                            // renumbering pads the tail of each slice)
  bool directed = false, weighted = false, has_in = false;
  uint64_t local_edges = 0, total_edges = 0, input_edges = 0;
  std::vector<uint32_t> seg_host;
  DeviceBuffer<uint32_t> seg;
  DeviceBuffer<uint64_t> oe_off;
  DeviceBuffer<uint32_t> oe_dst;
  DeviceBuffer<float> oe_w;
  DeviceBuffer<uint64_t> ie_off;
  DeviceBuffer<uint32_t> ie_dst;
  DeviceBuffer<float> ie_w;
  // degree buckets over owned rows (built lazily; row-per-thread/wave/block
  // scheduling for whole-graph sweeps — the CTA scheduler, preprocessed)
  // Rows with no pull edge are in no bucket: a PageRank pull sums nothing
  // for them and a BFS pull can find them no parent.
  DeviceBuffer<uint32_t> rows_small, rows_mid, rows_large;
  uint64_t n_small = 0, n_mid = 0, n_large = 0;
  // rows_active: ascending owned rows with an edge in the pull CSR or the
  // out-CSR; its complement is the isolated set, whose PageRank follows a
  // scalar recurrence. Padding rows (>= owned_real) carry no edges
  // (upload pads their offsets flat), so they are never active and never
  // counted in n_isolated_real.
  DeviceBuffer<uint32_t> rows_active;
  uint64_t n_active = 0, n_isolated_real = 0, n_isolated_pad = 0;
  // the same set as a bitmap over the owned rows (bit r % 32 of word r / 32),
  // kept for pr_fill_isolated_kernel: one bit per row instead of two offsets
  DeviceBuffer<uint32_t> active_bm;
  // hub work list: every rows_large row cut into kHubSeg-arc items, in row
  // order. hub_item_row[i] indexes rows_large, hub_item_seg[i] is the
  // segment within the row, hub_row_first[j] the first item of row j
  // (n_large + 1 entries). pr_hub_part holds one fp64 partial per item.
  // All built with the buckets and alive as long as the graph: the cached
  // PageRank hipGraph bakes their pointers.
  DeviceBuffer<uint32_t> hub_item_row, hub_item_seg, hub_row_first;
  DeviceBuffer<double> pr_hub_part;
  uint64_t n_hub_items = 0;
  bool buckets_built = false;
  // PageRank id segments (ensure_pr_segments; layout in dev_graph.hpp).
  // seg_rows: the mid and hub rows, ascending. Per span, segment-major:
  // arc prefix, CSR base, index into seg_rows, first partial. A span that
  // crosses k items owns k consecutive partials; a row's partials are
  // contiguous in (segment, item) order from seg_row_first[row]. Built once
  // per graph and alive as long as it (the captured hipGraph bakes the
  // pointers). pr_seg_state: 0 undecided, 1 built and used, -1 off.
  DeviceBuffer<uint32_t> seg_rows, seg_span_row, seg_span_slot, seg_ctr;
  DeviceBuffer<uint64_t> seg_span_pref, seg_span_base, seg_row_first;
  DeviceBuffer<double> seg_part;
  // arcs of seg_rows[j], for the reduce's epilogue (KERNELS.md "PageRank
  // epilogues"): 4 B per row, read in row order
  DeviceBuffer<uint32_t> seg_row_deg;
  uint64_t n_seg_rows = 0, n_seg_spans = 0, n_seg_parts = 0;
  uint32_t seg_bound[kPrSegs + 1] = {};
  PrSegView seg_view{};
  int pr_seg_state = 0;
  double pr_seg_build_ms = 0;
  // mirror topology (multi-GPU, built lazily): the reference's mirror-info /
  // BatchShuffle design (edgecut_fragment_base.h:569+, cuda batch_shuffle
  // :81-103) recast for xGMI — per-peer sorted lists of the REMOTE vertices
  // this rank's edges actually reference (recv side) and of the OWNED
  // vertices each peer references (send side). Dense per-round refreshes
  // then ship referenced values point-to-point on distinct xGMI links
  // instead of allgathering whole slices around the ring.
  DeviceBuffer<uint32_t> mr_recv_idx, mr_send_idx;   // concatenated, global ids
  std::vector<uint64_t> mr_recv_off, mr_send_off;    // [world+1] element offs
  DeviceBuffer<uint8_t> mr_sendbuf, mr_recvbuf;      // 4B-element staging
  bool mirrors_built = false;
  // CDLP label order (non-identity maps only): dev id -> rank in global
  // sorted-OID order, so min-label tie-breaks match the reference's
  // oid-space semantics under dense renumbering. Empty for identity maps.
  DeviceBuffer<uint32_t> oid_order;
  // hub-clustering renumber (synthetic graphs): new = perm[old],
  // old = inv[new]; slices preserved. inv_host caches the owned slice
  // for output oid translation (filled on first fetch).
  DeviceBuffer<uint32_t> perm, inv;
  bool permuted = false;
  std::vector<uint32_t> inv_host;
  // PageRank tiled-pull stream (built lazily; 8 B per stored edge):
  // (src<<32|dst) records grouped by 4096-vertex dst tile so gathers stay
  // L2-resident. pr_ntiles==0 after build => fell back (memory gate).
  DeviceBuffer<unsigned long long> pr_tiles;
  DeviceBuffer<uint64_t> pr_tile_off;
  uint32_t pr_ntiles = 0;
  uint64_t pr_own_lo = 0, pr_own_hi = 0, pr_total = 0;
  bool pr_tiles_built = false;
  uint32_t owned() const { return v_end - v_begin; }
  // cached hipGraph of one PageRank iteration (single-GPU fixed-iter
  // path) + the working set it references: the capture bakes device
  // pointers, so these buffers must live as long as the graph
  void* pr_graph_exec = nullptr;
  double pr_graph_damping = 0.0;
  int pr_calls = 0;  // capture lazily: one-shot runs skip the ~10ms
                     // instantiate; repeated runs (bench warmup) get it
  // pr_dangling: [0]=current dangling sum, [1]=next, [2]=previous base
  DeviceBuffer<double> pr_rank, pr_acc, pr_dangling;
  DeviceBuffer<float> pr_contrib;
  // Epilogue path (pagerank_epilogue; undirected, single GPU, fixed
  // iterations): the pulls apply the row sum themselves, so an iteration
  // gathers from one contribution buffer and writes the other. pr_contrib2
  // is allocated when the path first runs, pr_acc only when another path
  // does. pr_epi_scal: [0]=dangling sum, [1]=base of the iteration,
  // [2]=previous base. pr_epi_exec: the captured iteration pr_contrib ->
  // pr_contrib2 [0] and back [1]; neither writes pr_rank.
  DeviceBuffer<float> pr_contrib2;
  DeviceBuffer<double> pr_epi_scal;
  void* pr_epi_exec[2] = {nullptr, nullptr};
  double pr_epi_damping = 0.0;
  // random-walk sampler indexes (built lazily by sample(), kept with the
  // graph). sample_cdf: inclusive fp32 prefix sum of the weights inside each
  // stored out-row, 4 B per stored arc (edge_weight on weighted graphs).
  // Top-k index for one k at a time (top_k on weighted graphs), only for
  // rows longer than k: sample_topk_rank[r] = how many such rows precede
  // row r (8 B per owned row), sample_topk_slots[rank * k + j] = row slot of
  // the j-th heaviest arc, ties to the smaller slot (4 * k B per such row).
  DeviceBuffer<float> sample_cdf;
  bool sample_cdf_built = false;
  DeviceBuffer<uint64_t> sample_topk_rank;
  DeviceBuffer<uint32_t> sample_topk_slots;
  int sample_topk_k = 0;  // 0: no index yet
  ~DeviceGraph();
};

struct GpuRunResult {
  std::vector<int64_t> i64;   // BFS depth / WCC & CDLP labels (owned range)
  std::vector<double> f64;    // SSSP dist / PR rank / LCC coeff / BC delta
  std::vector<double> f64b;   // BC path counts (sigma); empty otherwise
  int rounds = 0;
  double seconds = 0;         // max over ranks, kernel-side barrier-bracketed
  uint64_t traversed_edges = 0;  // for TEPS accounting (global)
  // this rank's data-plane sends during the run (comm-volume evidence:
  // p2p halo/mirror/row-fetch vs collective traffic)
  uint64_t bytes_p2p = 0, bytes_coll = 0;
  uint64_t count = 0;  // kclique: the global number of k-cliques
  // sample: indices into `starts` of the walks that begin on an owned
  // vertex, ascending, and their paths, [walk_ids.size()][hops + 1] device
  // ids of the graph as it was loaded (hub renumbering undone), 0xFFFFFFFF
  // from the first dead end on
  std::vector<int64_t> walk_ids;
  std::vector<uint32_t> paths;
};

// largest k of the device kclique (its mask stack is k - 2 registers deep)
constexpr int kCliqueMaxK = 8;
// largest top_k of the device sampler (the index is built by top_k arg-max
// passes over a row)
constexpr int kSampleTopKMax = 32;
// a start of sample() that is no vertex of the graph
constexpr uint32_t kSampleNoVertex = 0xFFFFFFFFu;

class GpuContext {
 public:
  GpuContext(TcpComm* comm, int rank, int world);
  ~GpuContext();

  // Build a device graph from a host fragment (identity vertex map only).
  std::unique_ptr<DeviceGraph> upload(const Fragment& frag);

  // Generate an LDBC-datagen-shaped synthetic graph directly in HBM3E
  // (RMAT skew, random [1,100) weights), one owned slice per rank.
  std::unique_ptr<DeviceGraph> gen_synthetic(uint64_t nv, uint64_t ne,
                                             uint64_t seed, bool directed,
                                             bool weighted, bool build_in_csr,
                                             double rmat_a, double rmat_b,
                                             double rmat_c);

  // fetch=false skips the result D2H/convert (bench times algorithm only,
  // like the reference's "run algorithm" timer phase vs the Output phase).
  GpuRunResult bfs(DeviceGraph& g, int64_t source, bool fetch = true);
  GpuRunResult sssp(DeviceGraph& g, int64_t source, float delta,
                    bool fetch = true);
  GpuRunResult pagerank(DeviceGraph& g, double damping, int iters,
                        double tol = 0.0, bool fetch = true);
  GpuRunResult wcc(DeviceGraph& g, bool fetch = true);
  GpuRunResult cdlp(DeviceGraph& g, int iters, bool fetch = true);
  GpuRunResult lcc(DeviceGraph& g, bool fetch = true);
  GpuRunResult lcc_directed(DeviceGraph& g, bool fetch = true);
  // frontier peeling on the stored out-CSR (cpp/apps/kcore.hpp semantics)
  // i64: 1 = in the k-core, 0 = peeled
  GpuRunResult kcore(DeviceGraph& g, int k, bool fetch = true);
  // i64: coreness
  GpuRunResult core_decomposition(DeviceGraph& g, bool fetch = true);
  // single-source Brandes on the stored out-CSR (cpp/apps/bc.hpp semantics)
  // f64: dependency delta, f64b: path counts, i64: depth; rounds: levels
  GpuRunResult bc(DeviceGraph& g, int64_t source, bool fetch = true);
  // k-cliques of an undirected graph, 2 <= k <= kCliqueMaxK, by bitmap
  // enumeration over the degree-oriented CSR; count: the global total on
  // every rank
  GpuRunResult kclique(DeviceGraph& g, int k);
  // random walks of `hops` steps on the stored out-CSR, one per entry of
  // `starts` (device ids of the graph as loaded, kSampleNoVertex for a start
  // that is no vertex; every rank passes the same list). strategy: 0 random,
  // 1 edge_weight, 2 top_k (cpp/apps/sampler.hpp SampleStrategy). The draw
  // of a step depends on (seed, index into starts, hop) alone. rounds: hops
  // that still had a live walk; traversed_edges: steps taken, global.
  GpuRunResult sample(DeviceGraph& g, const std::vector<uint32_t>& starts,
                      int hops, int strategy, int top_k, uint64_t seed);
  // fan-out (neighbourhood) sampling on the stored out-CSR: fanouts[0]
  // neighbours of every seed, fanouts[1] of each of those, ..., drawn with
  // replacement by the draw and pick rule of sample() with the sample slot
  // in place of the hop (core/fanout.hpp has the layout). seeds as `starts`
  // of sample(). walk_ids: the owned seeds; paths: their rows,
  // [walk_ids.size()][1 + S], 0xFFFFFFFF below a dead end. rounds: levels
  // that began with a live parent somewhere; traversed_edges: samples
  // drawn, global. Throws on a table above kFanoutMaxEntries.
  // replace = false: the children of a parent are distinct arc slots, all of
  // its domain where that is no longer than the fan-out (core/fanout.hpp has
  // the rule). random and top_k only: edge_weight on a weighted graph throws,
  // and so does a fan-out above kFanoutNoReplaceMax.
  GpuRunResult sample_neighbors(DeviceGraph& g,
                                const std::vector<uint32_t>& seeds,
                                const std::vector<int64_t>& fanouts,
                                int strategy, int top_k, uint64_t seed,
                                bool replace = true);

  void device_sync();
  // test hook: exclusive scan of host u32 data on the device
  std::vector<uint64_t> debug_scan(const std::vector<uint32_t>& in);
  // test hook: segmented sort of host CSR rows on the device; returns the
  // sorted dst. w null: u32 keys; w given: (dst, weight) pairs, w sorted in
  // place along with dst.
  std::vector<uint32_t> debug_sort_rows(const std::vector<uint64_t>& off,
                                        std::vector<uint32_t> dst,
                                        std::vector<float>* w);
  // test hook: frontier-expansion launches so far per scheduler, in the
  // order cm, wm, strict, none (host-side count; expand_cm_range is no
  // scheduler choice and is not counted). reset zeroes them after the read.
  std::array<uint64_t, 4> debug_expand_counts(bool reset = false);
  // test hook: pagerank() calls so far whose mid and hub rows went through
  // the id-segment pull [0] or the row-tier pulls [1] (single-GPU row pull
  // only; the tiled and multi-GPU paths count as neither)
  std::array<uint64_t, 2> debug_pr_path(bool reset = false);
  // test hook: pagerank() calls so far that took the epilogue path [0] and
  // the iterations of those calls that were replayed from a captured
  // hipGraph [1] (GRAPEHIP_PR_EPILOGUE, read once per process)
  std::array<uint64_t, 2> debug_pr_epilogue(bool reset = false);
  // test hook: the arc depth in effect (GRAPEHIP_ARC_DEPTH, read once per
  // process; KERNELS.md "Arc depth")
  int debug_arc_depth();
  // test hook: device kclique() calls so far, the rows of the last call in
  // the wave, block and global tiers, kCliqueBlockMax and kCliqueMaxK, in
  // that order. reset zeroes the first four after the read.
  std::array<uint64_t, 6> debug_kclique(bool reset = false);
  // test hook: device sample() calls, cdf and top-k index builds so far,
  // the steps of the last call, and the bytes and build time of the last
  // index built of each kind; sample_neighbors() calls and the draws of the
  // last one. reset zeroes the counts after the read.
  struct SampleDebug {
    uint64_t calls = 0, cdf_builds = 0, topk_builds = 0, steps = 0;
    uint64_t fanout_calls = 0, fanout_draws = 0;
    uint64_t cdf_bytes = 0, topk_bytes = 0;
    double cdf_ms = 0, topk_ms = 0;
  };
  SampleDebug debug_sample(bool reset = false);
  // test hook: the id-segment layout of g, built if it is not yet (empty
  // rows when the path is off for g), with the pull CSR it was cut from
  struct PrSegDebug {
    bool on = false;
    uint32_t item = 0;
    std::vector<uint32_t> bound, rows, span_row, span_slot;
    std::vector<uint64_t> span_first, span_pref, span_base, row_first;
    std::vector<uint64_t> off;
    std::vector<uint32_t> dst;
    double build_ms = 0;
    uint64_t bytes = 0;
  };
  PrSegDebug debug_pr_segments(DeviceGraph& g);
  // test hook: the stored graph of g as it lies on the device, in stored
  // ids: row r of off/in_off is vertex v_begin + r. The in arrays are empty
  // without an in-CSR, w/in_w on an unweighted graph, old_of_new/new_of_old
  // (inv/perm) on a graph that is not hub-renumbered. Copies only; world 1.
  struct CsrDebug {
    uint32_t v_begin = 0;
    bool weighted = false, has_in = false, permuted = false;
    std::vector<uint64_t> off, in_off;
    std::vector<uint32_t> dst, in_dst, old_of_new, new_of_old;
    std::vector<float> w, in_w;
  };
  CsrDebug debug_csr(const DeviceGraph& g);
  int device_id() const { return dev_; }
  TcpComm* comm() { return comm_; }
  int rank() const { return rank_; }
  int world() const { return world_; }

  struct Impl;  // internal (kernels + scratch); public for free helpers

 private:
  // shared peeling driver: all levels (coreness) or the single level k - 1
  GpuRunResult peel(DeviceGraph& g, bool all_levels, int k, bool fetch);
  // pagerank() on the epilogue path; seg: the id-segment pull is on for g
  GpuRunResult pagerank_epilogue(DeviceGraph& g, double damping, int iters,
                                 bool seg, bool fetch);
  std::unique_ptr<Impl> impl_;
  TcpComm* comm_;
  int rank_, world_, dev_ = 0;
};

}  // namespace grapehip
