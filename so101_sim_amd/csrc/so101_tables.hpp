// Host-side builders of the per-hull tables that so101_create() and so101_tree_create() upload (so101_model.hpp DevModel::hull_sbt,
// hl_entry / hl_off).  One copy for both engines and for the device probes of the test suite (tests/devprims), which check these tables
// against an fp64 brute force.  V: the hull's n >= 1 vertices, xyz interleaved (the floats of the blob's mesh_vert).
#pragma once
#include "so101_model.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// support-bound table of one hull (DevModel::hull_sbt): out[SBT_DIM], in double, rounded up to float
inline void build_support_bounds(const float* V, int n, float* out) {
  for (int face = 0; face < 6; face++) {
    int ax = face / 2; double sg = (face & 1) ? -1.0 : 1.0;
    for (int iu = 0; iu < SBT_GRID; iu++)
      for (int iv = 0; iv < SBT_GRID; iv++) {
        const double step = 2.0 / (SBT_GRID - 1);
        double c[3]; c[ax] = sg; c[(ax + 1) % 3] = -1.0 + step * iu; c[(ax + 2) % 3] = -1.0 + step * iv;
        double best = -1e300;
        for (int k = 0; k < n; k++) best = std::max(best, (double)V[3 * k] * c[0] + (double)V[3 * k + 1] * c[1] + (double)V[3 * k + 2] * c[2]);
        float f = (float)best;
        if ((double)f < best) f = std::nextafterf(f, 3.0e38f);
        out[(face * SBT_GRID + iu) * SBT_GRID + iv] = f;
      }
  }
}

// support-vertex lists of one hull (DevModel::hl_entry / hl_off): appends the entries of its HL_CELLS cells to `entries` (four floats each) and
// writes off[0 .. HL_CELLS], the cells' ranges in units of entries counted from the start of `entries`
inline void build_support_lists(const float* V, int n, std::vector<float>& entries, unsigned int* off) {
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int k = 0; k < n; k++) for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], (double)V[3 * k + a]); hi[a] = std::max(hi[a], (double)V[3 * k + a]); }
  const double diam = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
  std::vector<double> S((size_t)(HL_GRID + 1) * (HL_GRID + 1) * n);          // scores of every vertex at the grid points of one face
  std::vector<double> cn((size_t)(HL_GRID + 1) * (HL_GRID + 1));
  for (int face = 0; face < 6; face++) {
    int ax = face / 2; double sg = (face & 1) ? -1.0 : 1.0;
    for (int iu = 0; iu <= HL_GRID; iu++)
      for (int iv = 0; iv <= HL_GRID; iv++) {
        double c[3]; c[ax] = sg; c[(ax + 1) % 3] = -1.0 + 2.0 * iu / HL_GRID; c[(ax + 2) % 3] = -1.0 + 2.0 * iv / HL_GRID;
        size_t pt = (size_t)iu * (HL_GRID + 1) + iv;
        cn[pt] = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        double* sp = &S[pt * n];
        for (int k = 0; k < n; k++) sp[k] = V[3 * k] * c[0] + V[3 * k + 1] * c[1] + V[3 * k + 2] * c[2];
      }
    for (int iu = 0; iu < HL_GRID; iu++)
      for (int iv = 0; iv < HL_GRID; iv++) {
        const size_t pts[4] = {(size_t)iu * (HL_GRID + 1) + iv, (size_t)(iu + 1) * (HL_GRID + 1) + iv, (size_t)iu * (HL_GRID + 1) + iv + 1, (size_t)(iu + 1) * (HL_GRID + 1) + iv + 1};
        int win[4]; double eps[4];
        for (int q = 0; q < 4; q++) {
          const double* sp = &S[pts[q] * n]; int w = 0;
          for (int k = 1; k < n; k++) if (sp[k] > sp[w]) w = k;
          win[q] = w; eps[q] = 4e-3 * diam * cn[pts[q]] + 1e-6;
        }
        off[(face * HL_GRID + iu) * HL_GRID + iv] = (unsigned int)(entries.size() / 4);
        for (int k = 0; k < n; k++) {
          bool keep = true;
          for (int w = 0; w < 4 && keep; w++) {            // beaten by corner winner w at ALL four corners by more than the widening: out
            bool some = false;
            for (int q = 0; q < 4; q++) some = some || S[pts[q] * n + k] >= S[pts[q] * n + win[w]] - eps[q];
            keep = some;
          }
          if (keep) { entries.push_back(V[3 * k]); entries.push_back(V[3 * k + 1]); entries.push_back(V[3 * k + 2]); float fi; unsigned int ui = (unsigned int)k; memcpy(&fi, &ui, 4); entries.push_back(fi); }
        }
      }
  }
  off[HL_CELLS] = (unsigned int)(entries.size() / 4);
}
