// grapehip — GNN random-walk sampler, CPU path.
// Reference parity: examples/gnn_sampler/sampler.h:35-238 (multi-hop walks
// from query vertices, strategies random / edge_weight / top_k via
// per-vertex index structures, fragment_indices.h) as a ParallelApp over
// the BSP engine: each round advances every live walk one hop; walks whose
// current vertex is remote travel to its owner as (walk, hop, gid)
// messages, and every sampled step is reported back to the walk's origin
// fragment the same way. Kafka streaming in/out (kafka_consumer.h) is not
// available in this environment; the Python driver replays edge streams
// through mutate_graph instead. FanoutSamplerApp below is the reference's
// --hop_and_num query (fan-out neighbourhood sampling) over the same engine.
#pragma once

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../core/fanout.hpp"
#include "../core/fragment.hpp"
#include "../core/message_manager.hpp"

namespace grapehip {

enum class SampleStrategy : int { kRandom = 0, kEdgeWeight = 1, kTopK = 2 };

// Per-vertex alias tables for O(1) weighted draws (reference
// fragment_indices.h builds the same structure per vertex). Flat over the
// fragment's edge-id space; built once per query in parallel.
struct AliasTables {
  std::vector<float> prob;     // [local eid]
  std::vector<uint32_t> alias; // [local eid] (intra-row index)

  void build(const Fragment& frag) {
    size_t ne = frag.local_edges();
    prob.assign(ne, 1.0f);
    alias.assign(ne, 0);
    parallel_for(0, frag.ivnum(), [&](size_t vs) {
      vid_t v = static_cast<vid_t>(vs);
      auto adj = frag.out_edges(v);
      if (adj.n == 0) return;
      size_t base = adj.dst - frag.oe_dsts().data();
      // Vose's method over the row's weights
      double total = 0;
      for (size_t i = 0; i < adj.n; ++i)
        total += adj.w ? adj.w[i] : 1.0;
      std::vector<double> scaled(adj.n);
      std::vector<uint32_t> small, large;
      for (size_t i = 0; i < adj.n; ++i) {
        scaled[i] = (adj.w ? adj.w[i] : 1.0) * adj.n / total;
        (scaled[i] < 1.0 ? small : large).push_back(
            static_cast<uint32_t>(i));
      }
      while (!small.empty() && !large.empty()) {
        uint32_t s = small.back();
        small.pop_back();
        uint32_t l = large.back();
        large.pop_back();
        prob[base + s] = static_cast<float>(scaled[s]);
        alias[base + s] = l;
        scaled[l] = scaled[l] + scaled[s] - 1.0;
        (scaled[l] < 1.0 ? small : large).push_back(l);
      }
      for (uint32_t i : large) prob[base + i] = 1.0f;
      for (uint32_t i : small) prob[base + i] = 1.0f;
    }, 256);
  }
};

struct SamplerContext {
  SampleStrategy strategy = SampleStrategy::kRandom;
  int hops = 2;
  int top_k = 4;
  uint64_t seed = 7;
  AliasTables alias;  // built when strategy == kEdgeWeight
  // walks this fragment OWNS (origin here); path[w][h], gid space,
  // kInvalidVid where the walk died (dead end)
  std::vector<uint64_t> walk_ids;            // global walk index
  std::vector<std::vector<vid_t>> paths;     // [local walk][hops+1]
  // walks currently AT this fragment: (walk id, hop just reached, vertex)
  struct Live {
    uint64_t walk;
    int hop;
    vid_t gid;
  };
  std::vector<Live> live;

  void init(const Fragment& frag, const std::vector<oid_t>& starts,
            int hops_, SampleStrategy st, int k, uint64_t seed_) {
    strategy = st;
    hops = hops_;
    top_k = k;
    seed = seed_;
    walk_ids.clear();
    paths.clear();
    live.clear();
    for (size_t i = 0; i < starts.size(); ++i) {
      vid_t lid;
      if (frag.oid2lid(starts[i], &lid) && frag.inner(lid)) {
        vid_t g = frag.lid2gid(lid);
        walk_ids.push_back(i);
        std::vector<vid_t> p(hops + 1, kInvalidVid);
        p[0] = g;
        paths.push_back(std::move(p));
        live.push_back({i, 0, g});
      }
    }
  }
};

class SamplerApp {
 public:
  struct Msg {
    uint64_t walk;
    int32_t hop;     // hop index of `gid` in the walk
    int32_t record;  // 1 = report to origin's path, 0 = advance here
    vid_t gid;
  };

  void PEval(const Fragment& frag, SamplerContext& ctx, MessageManager& mm) {
    if (ctx.strategy == SampleStrategy::kEdgeWeight)
      ctx.alias.build(frag);
    advance(frag, ctx, mm);
  }

  void IncEval(const Fragment& frag, SamplerContext& ctx,
               MessageManager& mm) {
    // collect arrivals + records
    std::vector<SamplerContext::Live> arrivals;
    mm.process_raw<Msg>([&](int, vid_t, Msg m) {
      if (m.record) {
        rec_mutex_.lock();
        records_.push_back(m);
        rec_mutex_.unlock();
      } else {
        arr_mutex_.lock();
        arrivals.push_back({m.walk, m.hop, m.gid});
        arr_mutex_.unlock();
      }
    });
    // apply records to owned paths (walk origin == this fragment)
    for (const Msg& m : records_) {
      auto it = std::lower_bound(ctx.walk_ids.begin(), ctx.walk_ids.end(),
                                 m.walk);
      if (it != ctx.walk_ids.end() && *it == m.walk)
        ctx.paths[it - ctx.walk_ids.begin()][m.hop] = m.gid;
    }
    records_.clear();
    // arrivals JOIN the locally-advancing walks (replacing them dropped
    // every local walk after its first hop)
    ctx.live.insert(ctx.live.end(), arrivals.begin(), arrivals.end());
    advance(frag, ctx, mm);
  }

 private:
  std::mutex rec_mutex_, arr_mutex_;
  std::vector<Msg> records_;

  template <typename RNG>
  vid_t sample_neighbor(const Fragment& frag, const SamplerContext& ctx,
                        vid_t lid, RNG& rng) const {
    auto adj = frag.out_edges(lid);
    if (adj.n == 0) return kInvalidVid;
    size_t pick = 0;
    switch (ctx.strategy) {
      case SampleStrategy::kRandom:
        pick = rng() % adj.n;
        break;
      case SampleStrategy::kEdgeWeight: {
        // O(1) alias draw (Vose): pick a slot, then flip against its prob
        size_t base = adj.dst - frag.oe_dsts().data();
        size_t slot = rng() % adj.n;
        double coin = static_cast<double>(rng() & 0xFFFFFFFFFFFFull) /
                      double(0x1000000000000ull);
        pick = coin < ctx.alias.prob[base + slot]
                   ? slot
                   : ctx.alias.alias[base + slot];
        break;
      }
      case SampleStrategy::kTopK: {
        // uniform among the k heaviest edges (ties by dst gid for
        // determinism, like the reference's sorted index)
        size_t k = std::min<size_t>(ctx.top_k, adj.n);
        std::vector<size_t> idx(adj.n);
        for (size_t i = 0; i < adj.n; ++i) idx[i] = i;
        std::partial_sort(idx.begin(), idx.begin() + k, idx.end(),
                          [&](size_t a, size_t b) {
                            float wa = adj.w ? adj.w[a] : 1.0f;
                            float wb = adj.w ? adj.w[b] : 1.0f;
                            if (wa != wb) return wa > wb;
                            return frag.lid2gid(adj.dst[a]) <
                                   frag.lid2gid(adj.dst[b]);
                          });
        pick = idx[rng() % k];
        break;
      }
    }
    return frag.lid2gid(adj.dst[pick]);
  }

  void advance(const Fragment& frag, SamplerContext& ctx,
               MessageManager& mm) {
    bool any_live = false;
    for (const auto& lv : ctx.live) {
      if (lv.hop >= ctx.hops) continue;
      vid_t lid = frag.gid2lid(lv.gid);
      if (lid == kInvalidVid || !frag.inner(lid)) continue;
      // per-(walk, hop) deterministic RNG stream
      std::mt19937_64 rng(ctx.seed * 0x9e3779b97f4a7c15ULL + lv.walk * 1000003ULL +
                          static_cast<uint64_t>(lv.hop));
      vid_t nxt = sample_neighbor(frag, ctx, lid, rng);
      if (nxt == kInvalidVid) continue;  // dead end: walk stops
      int nhop = lv.hop + 1;
      // record the step at the walk's origin
      fid_t origin = origin_of(frag, ctx, lv.walk);
      if (origin == frag.fid()) {
        auto it = std::lower_bound(ctx.walk_ids.begin(), ctx.walk_ids.end(),
                                   lv.walk);
        ctx.paths[it - ctx.walk_ids.begin()][nhop] = nxt;
      } else {
        mm.send_to_fragment(0, origin, /*routing gid (unused)*/ 0,
                            Msg{lv.walk, nhop, 1, nxt});
      }
      // advance the walk
      if (nhop < ctx.hops) {
        fid_t owner = frag.parser().fid(nxt);
        if (owner == frag.fid()) {
          next_live_.push_back({lv.walk, nhop, nxt});
          any_live = true;
        } else {
          mm.send_to_fragment(0, owner, nxt, Msg{lv.walk, nhop, 0, nxt});
          any_live = true;
        }
      }
    }
    ctx.live = std::move(next_live_);
    next_live_.clear();
    if (any_live || !ctx.live.empty()) mm.force_continue();
  }

  fid_t origin_of(const Fragment& frag, const SamplerContext& ctx,
                  uint64_t walk) const {
    // walks are issued per-origin; origin = owner of the start vertex.
    // The start oid isn't carried, so the origin is resolved from the walk
    // table replicated at init: ranks only look up walks they own, and
    // remote records carry the origin in origin_map_.
    return origin_map_.empty() ? frag.fid()
                               : origin_map_[walk];
  }

 public:
  // set by the driver before Query: owner fragment of each walk's start
  std::vector<fid_t> origin_map_;

 private:
  std::vector<SamplerContext::Live> next_live_;
};

// ---------------------------------------------------------------------------
// Fan-out (neighbourhood) sampling, CPU path. Reference parity:
// examples/gnn_sampler --hop_and_num f_1-...-f_H (sampler.h hop_size /
// next_pos): f_1 neighbours of every seed, f_2 of each of those, ..., with
// replacement, or as distinct arcs of the parent (replace = false), one flat
// row of 1 + S ids per seed (core/fanout.hpp).
//
// The draws are those of the device path (hip/gpu_engine.hip sample_draw and
// sample_pick), so host, device and the NumPy oracle agree entry for entry:
// the draw of sample slot pos of seed index i is draw(seed, i, pos), taken
// out of the parent's out-row in stored order, which is ascending gid (the
// device's ascending device id).
// ---------------------------------------------------------------------------

inline uint64_t fanout_draw(uint64_t seed, uint64_t walk, uint64_t hop) {
  uint64_t x = seed * 0x9E3779B97F4A7C15ULL + walk * 0xD1B54A32D192ED03ULL +
               hop;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}

inline uint64_t fanout_mulhi(uint64_t a, uint64_t b) {
  return static_cast<uint64_t>(
      (static_cast<unsigned __int128>(a) * b) >> 64);
}

struct FanoutContext {
  SampleStrategy strategy = SampleStrategy::kRandom;
  int top_k = 4;
  uint64_t seed = 7;
  bool replace = true;  // false: distinct arc slots per parent
  FanoutLayout lay;
  int level = 0;  // the level the live nodes sit on
  // the out-rows of the inner vertices in stored order (ascending gid,
  // parallel arcs in fragment order); cdf: inclusive fp32 prefix sum of a
  // row's weights, built for edge_weight on a weighted fragment
  std::vector<eid_t> off;
  std::vector<vid_t> nbr;  // gids
  std::vector<float> w, cdf;
  // seeds this fragment OWNS; nodes[s * row_len + column], gid space,
  // kInvalidVid for none
  std::vector<uint64_t> seed_ids;
  std::vector<vid_t> nodes;
  // tree nodes currently AT this fragment: (seed index, column, vertex)
  struct Live {
    uint64_t seed;
    uint64_t col;
    vid_t gid;
  };
  std::vector<Live> live;

  void init(const Fragment& frag, const std::vector<oid_t>& seeds,
            const std::vector<int64_t>& fanouts, SampleStrategy st, int k,
            uint64_t seed_, bool replace_ = true) {
    lay = fanout_layout(fanouts, seeds.size());  // throws before any alloc
    if (!replace_)
      fanout_check_no_replace(st == SampleStrategy::kEdgeWeight &&
                              frag.has_weights());
    if (st == SampleStrategy::kTopK && k < 1)
      throw std::runtime_error("sample_neighbors: top_k = " +
                               std::to_string(k) + " is below 1");
    strategy = st;
    top_k = k;
    seed = seed_;
    replace = replace_;
    level = 0;
    seed_ids.clear();
    live.clear();
    for (size_t i = 0; i < seeds.size(); ++i) {
      vid_t lid;
      if (frag.oid2lid(seeds[i], &lid) && frag.inner(lid)) {
        seed_ids.push_back(i);
        live.push_back({i, 0, frag.lid2gid(lid)});
      }
    }
    const uint64_t row_len = lay.row_len();
    nodes.assign(seed_ids.size() * row_len, kInvalidVid);
    for (size_t s = 0; s < seed_ids.size(); ++s)
      nodes[s * row_len] = live[s].gid;
  }

  void build_rows(const Fragment& frag) {
    const vid_t iv = frag.ivnum();
    off.assign(static_cast<size_t>(iv) + 1, 0);
    for (vid_t v = 0; v < iv; ++v) off[v + 1] = off[v] + frag.out_degree(v);
    nbr.resize(off[iv]);
    const bool weighted = frag.has_weights();
    const bool want_cdf = weighted && strategy == SampleStrategy::kEdgeWeight;
    if (weighted) w.resize(off[iv]); else w.clear();
    if (want_cdf) cdf.resize(off[iv]); else cdf.clear();
    parallel_for(0, iv, [&](size_t vs) {
      auto adj = frag.out_edges(static_cast<vid_t>(vs));
      if (adj.n == 0) return;
      const eid_t b = off[vs];
      std::vector<std::pair<vid_t, uint32_t>> key(adj.n);
      for (size_t i = 0; i < adj.n; ++i)
        key[i] = {frag.lid2gid(adj.dst[i]), static_cast<uint32_t>(i)};
      std::sort(key.begin(), key.end());
      float acc = 0.f;
      for (size_t i = 0; i < adj.n; ++i) {
        nbr[b + i] = key[i].first;
        if (weighted) w[b + i] = adj.w[key[i].second];
        if (want_cdf) cdf[b + i] = acc = acc + w[b + i];
      }
    }, 256);
  }

  // the child that draw r takes from inner vertex lid; kInvalidVid at a
  // dead end
  vid_t pick(vid_t lid, uint64_t r) const {
    const eid_t b = off[lid];
    const uint64_t deg = off[lid + 1] - b;
    if (deg == 0) return kInvalidVid;
    uint64_t slot = 0;
    if (strategy == SampleStrategy::kRandom ||
        (strategy == SampleStrategy::kEdgeWeight && cdf.empty())) {
      slot = fanout_mulhi(r, deg);
    } else if (strategy == SampleStrategy::kEdgeWeight) {
      const float* c = cdf.data() + b;
      const float total = c[deg - 1];
      if (!(total > 0.f)) return kInvalidVid;
      const float u =
          static_cast<float>(static_cast<uint32_t>(r >> 40)) * 0x1p-24f;
      const float t = u * total;  // one fp32 multiply, rounded to nearest
      slot = std::upper_bound(c, c + deg, t) - c;
      if (slot >= deg) slot = deg - 1;
    } else {
      const uint64_t k = static_cast<uint64_t>(top_k);
      const uint64_t kk = std::min<uint64_t>(k, deg);
      slot = fanout_mulhi(r, kk);
      if (!w.empty() && deg > k) {
        // the slot-th heaviest arc, ties to the smaller slot
        const float* wr = w.data() + b;
        std::vector<uint32_t> idx(deg);
        for (uint64_t i = 0; i < deg; ++i) idx[i] = static_cast<uint32_t>(i);
        std::partial_sort(idx.begin(), idx.begin() + kk, idx.end(),
                          [&](uint32_t x, uint32_t y) {
                            if (wr[x] != wr[y]) return wr[x] > wr[y];
                            return x < y;
                          });
        slot = idx[slot];
      }
    }
    return nbr[b + slot];
  }

  // replace = false: the f children of inner vertex lid together, children
  // [c] = kInvalidVid for none (core/fanout.hpp has the rule); draw_of(c) is
  // the draw of child c's sample slot
  template <typename Draw>
  void pick_distinct(vid_t lid, uint64_t f, Draw draw_of,
                     std::vector<vid_t>& children) const {
    children.assign(f, kInvalidVid);
    const eid_t b = off[lid];
    const uint64_t deg = off[lid + 1] - b;
    uint64_t m = deg;
    // the domain: element e is slot order[e], or slot e where order is empty
    std::vector<uint32_t> order;
    if (strategy == SampleStrategy::kTopK) {
      const uint64_t k = static_cast<uint64_t>(top_k);
      m = std::min<uint64_t>(k, deg);
      if (!w.empty() && deg > k) {
        const float* wr = w.data() + b;
        order.resize(deg);
        for (uint64_t i = 0; i < deg; ++i) order[i] = static_cast<uint32_t>(i);
        std::partial_sort(order.begin(), order.begin() + m, order.end(),
                          [&](uint32_t x, uint32_t y) {
                            if (wr[x] != wr[y]) return wr[x] > wr[y];
                            return x < y;
                          });
      }
    }
    auto element = [&](uint64_t e) {
      return nbr[b + (order.empty() ? e : order[e])];
    };
    if (m <= f) {
      for (uint64_t c = 0; c < m; ++c) children[c] = element(c);
      return;
    }
    // Floyd's subset sampling in child order
    std::vector<uint64_t> taken(f);
    for (uint64_t c = 0; c < f; ++c) {
      const uint64_t J = m - f + c;
      const uint64_t t = fanout_mulhi(draw_of(c), J + 1);
      const bool seen =
          std::find(taken.begin(), taken.begin() + c, t) != taken.begin() + c;
      taken[c] = seen ? J : t;
      children[c] = element(taken[c]);
    }
  }
};

class FanoutSamplerApp {
 public:
  struct Msg {
    uint64_t seed;
    uint64_t col;
    int32_t record;  // 1 = report to the seed's origin, 0 = expand here
    vid_t gid;
  };

  // set by the driver before the query: owner fragment of each seed
  std::vector<fid_t> origin_map_;

  void PEval(const Fragment& frag, FanoutContext& ctx, MessageManager& mm) {
    ctx.build_rows(frag);
    expand(frag, ctx, mm);
  }

  void IncEval(const Fragment& frag, FanoutContext& ctx,
               MessageManager& mm) {
    std::vector<Msg> in;
    mm.process_raw<Msg>([&](int, vid_t, Msg m) {
      std::lock_guard<std::mutex> lk(in_mutex_);
      in.push_back(m);
    });
    const uint64_t row_len = ctx.lay.row_len();
    for (const Msg& m : in) {
      if (m.record) {
        ctx.nodes[row_of(ctx, m.seed) * row_len + m.col] = m.gid;
      } else {
        ctx.live.push_back({m.seed, m.col, m.gid});
      }
    }
    expand(frag, ctx, mm);
  }

 private:
  std::mutex in_mutex_;

  static size_t row_of(const FanoutContext& ctx, uint64_t seed) {
    return std::lower_bound(ctx.seed_ids.begin(), ctx.seed_ids.end(), seed) -
           ctx.seed_ids.begin();
  }

  // one level: every live node draws its children
  void expand(const Fragment& frag, FanoutContext& ctx, MessageManager& mm) {
    const int h = ++ctx.level;
    std::vector<FanoutContext::Live> next;
    std::vector<vid_t> children;  // of one parent, replace = false
    if (h <= ctx.lay.levels()) {
      const uint64_t f = ctx.lay.fan[h - 1];
      const uint64_t row_len = ctx.lay.row_len();
      const bool more = h < ctx.lay.levels();
      for (const auto& nd : ctx.live) {
        const vid_t lid = frag.gid2lid(nd.gid);
        if (lid == kInvalidVid || !frag.inner(lid)) continue;
        const uint64_t first =
            ctx.lay.col[h] + (nd.col - ctx.lay.col[h - 1]) * f;
        const fid_t origin =
            origin_map_.empty() ? frag.fid() : origin_map_[nd.seed];
        const size_t row = origin == frag.fid() ? row_of(ctx, nd.seed) : 0;
        if (!ctx.replace)
          ctx.pick_distinct(lid, f, [&](uint64_t c) {
            return fanout_draw(ctx.seed, nd.seed, first + c - 1);
          }, children);
        for (uint64_t c = 0; c < f; ++c) {
          const uint64_t col = first + c;
          const vid_t child =
              ctx.replace
                  ? ctx.pick(lid, fanout_draw(ctx.seed, nd.seed, col - 1))
                  : children[c];
          if (child == kInvalidVid) continue;  // dead: the subtree stays -1
          if (origin == frag.fid())
            ctx.nodes[row * row_len + col] = child;
          else
            mm.send_to_fragment(0, origin, /*routing gid (unused)*/ 0,
                                Msg{nd.seed, col, 1, child});
          if (!more) continue;
          const fid_t owner = frag.parser().fid(child);
          if (owner == frag.fid())
            next.push_back({nd.seed, col, child});
          else
            mm.send_to_fragment(0, owner, child, Msg{nd.seed, col, 0, child});
        }
      }
    }
    ctx.live = std::move(next);
    if (!ctx.live.empty()) mm.force_continue();
  }
};

}  // namespace grapehip
