// grapehip — the table layout of fan-out (neighbourhood) sampling, shared by
// the host app (apps/sampler.hpp) and the device path (hip/gpu_engine.hip).
//
// Reference parity: examples/gnn_sampler/sampler.h hop_size offsets and
// next_pos (--hop_and_num f_1-...-f_H). Per seed one row of 1 + S ids:
// column 0 the seed, column 1 + pos sample slot pos. L_0 = 1,
// L_h = L_{h-1} * f_h, S = L_1 + ... + L_H; level h holds the slots
// base_h .. base_h + L_h - 1 with base_h = L_1 + ... + L_{h-1}, and slot
// base_h + j has its children in slots base_{h+1} + j * f_{h+1} + c.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace grapehip {

// largest table of one sample_neighbors call, n_seeds * (1 + S) entries:
// 2^31 ids are 8 GiB of device ids per rank and 16 GiB of int64 on the host
constexpr uint64_t kFanoutMaxEntries = 1ull << 31;

// Without replacement (replace=False) a live parent fills its f children
// from its *domain*, an ordered list of m arc slots of its stored out-row:
// the whole row in stored order (random; edge_weight without weights), or
// the min(deg, top_k) heaviest arcs, heaviest first, ties to the smaller slot
// (top_k). m <= f: child c < m takes domain element c, the others stay
// empty, no draw is used. m > f: Floyd's subset sampling in child order, with
// r_c the draw of child c's sample slot and index(r, n) = (r * n) >> 64:
//   J = m - f + c;  t = index(r_c, J + 1);
//   e_c = J if t is among e_0 .. e_{c-1}, else t;  child c takes element e_c.
// The e_c are distinct and every f-subset of the domain is equally likely.

// largest fan-out of the device path without replacement: one wave holds the
// picks of a parent
constexpr uint64_t kFanoutNoReplaceMax = 64;

// Weighted draws without replacement are not built; `weighted_draw`:
// strategy edge_weight on a graph that has weights.
inline void fanout_check_no_replace(bool weighted_draw) {
  if (weighted_draw)
    throw std::runtime_error(
        "sample_neighbors: strategy edge_weight with replace=False is not "
        "supported on a weighted graph (use random or top_k, or "
        "replace=True)");
}

struct FanoutLayout {
  std::vector<uint64_t> fan;  // [H] f_h
  std::vector<uint64_t> len;  // [H + 1] L_h
  std::vector<uint64_t> col;  // [H + 2] first column of level h; col[H+1] =
                              // 1 + S (the `level_offsets` of the result)
  uint64_t row_len() const { return col.back(); }
  int levels() const { return static_cast<int>(fan.size()); }
};

// Throws on a fan-out below 1 and on a table above kFanoutMaxEntries; the
// sizes are compared by division, so nothing overflows 64 bits.
inline FanoutLayout fanout_layout(const std::vector<int64_t>& fanouts,
                                  uint64_t n_seeds) {
  FanoutLayout lay;
  lay.len.push_back(1);
  lay.col = {0, 1};
  const uint64_t rows = n_seeds ? n_seeds : 1;
  const uint64_t max_row = kFanoutMaxEntries / rows;
  auto too_large = [&]() {
    std::string f;
    for (int64_t x : fanouts) f += (f.empty() ? "" : "-") + std::to_string(x);
    return std::runtime_error(
        "sample_neighbors: " + std::to_string(n_seeds) +
        " seeds with fanouts " + f + " need more than " +
        std::to_string(kFanoutMaxEntries) +
        " table entries (kFanoutMaxEntries)");
  };
  for (int64_t f : fanouts) {
    if (f < 1)
      throw std::runtime_error("sample_neighbors: fanout = " +
                               std::to_string(f) + " is below 1");
    const uint64_t uf = static_cast<uint64_t>(f);
    if (lay.len.back() > max_row / uf) throw too_large();
    const uint64_t L = lay.len.back() * uf;  // <= max_row
    if (lay.col.back() > max_row - L) throw too_large();
    lay.fan.push_back(uf);
    lay.len.push_back(L);
    lay.col.push_back(lay.col.back() + L);
  }
  if (lay.row_len() > max_row) throw too_large();
  return lay;
}

}  // namespace grapehip
