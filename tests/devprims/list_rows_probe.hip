// TEST HARNESS ONLY - device probe of k_narrow's list row pass (tu_narrow.hip), for tests/test_list_rows_emu.py and tests/test_list_rows_gpu.py.
// Built by tests/devprims/list_rows.py like support_probe.hip, which this file includes whole: the hull handle, its tables and the fused
// reference narrow_pair<NoCache, G64> (probe_pairs, mode 0) are the ones of that probe.
// One 64-lane workgroup works through `chunk` (1 .. 4) pairs at a time, one per DPP row of 16 lanes, the way the kernel does: the row takes the
// cell light_first_cell() names, loads the cell's list two entries per lane (hull_sub_row_load, the kernel's own loader) and runs
// narrow_pair_cached<HullSub, G16, true, true>.  Rows beyond the chunk stay idle, as the remainder rows of a short chunk do in the kernel.
#include "support_probe.hip"

namespace {

__global__ __launch_bounds__(64) void k_list_rows(const DevModel* m, int vnum, const float* pg, int nq, int chunk, int nblk, float* out) {
  const int lane = wave_lane(), row = lane >> 4;
  for (int i0 = chunk * (int)blockIdx.x; i0 < nq; i0 += chunk * nblk) {
    const int cnt = nq - i0 < chunk ? nq - i0 : chunk;
    if (row < cnt) {
      const int i = i0 + row;
      GeomW G1, G2; float rb1, rb2;
      pair_geoms(m, pg, i, vnum, G1, G2, rb1, rb2);
      PairContacts pc;
      pc.valid = 0u;
      for (int k = 0; k < 3; k++) pc.nrm[k] = 0.f;
      for (int q = 0; q < NCPP; q++) { pc.dist[q] = 0.f; for (int k = 0; k < 3; k++) pc.pos[q][k] = 0.f; }
      const int cell = light_first_cell(G1, G2);
      int a = 0, fcnt = 0;
      if (cell >= 0) { a = (int)m->hl_off[cell]; fcnt = (int)(m->hl_off[cell + 1] - m->hl_off[cell]); }
      float settled = -1.f;                            // (a list the row pass does not serve: none, or more than two entries per lane)
      if (fcnt >= 1 && fcnt <= HL_ROW_MAX) {
        HullSub S1, S2;
        hull_sub_row_load(m->hl_entry + 4 * (size_t)a, fcnt, S2);
#pragma unroll
        for (int q = 0; q < 2; q++) { S1.x[q] = 0.f; S1.y[q] = 0.f; S1.z[q] = 0.f; S1.i[q] = 0x7fffffff; }
        settled = narrow_pair_cached<HullSub, G16, true, true>(m, G1, G2, rb1, rb2, S1, S2, pc) ? 1.f : 0.f;
      }
      if ((lane & 15) == 0) pair_store(out + PAIR_OUT * i, settled, pc);
    }
  }
}

}  // namespace

extern "C" {

// the list row pass on nq (flat face, hull) pairs, `chunk` pairs per wavefront: arguments and output as probe_pairs
int probe_list_rows(void* h, int chunk, const float* pg, const float* rb, int nq, float* out) {
  Probe* p = (Probe*)h;
  if (!p || chunk < 1 || chunk > 4 || nq < 0) return -1;
  if (nq == 0) return 0;
  if (!inputs_ok(pg, PAIR_WORDS * (size_t)nq) || !inputs_ok(rb, 2 * (size_t)nq)) return -2;
  for (int i = 0; i < nq; i++) { int t = (int)pg[PAIR_WORDS * i]; if (t != G_PLANE && t != G_BOX) return -1; }
  DevBuf dg, dr, dm, dout;
  if (!dg.in(pg, PAIR_WORDS * (size_t)nq * sizeof(float)) || !dr.in(rb, 2 * (size_t)nq * sizeof(float)) || !dout.alloc(PAIR_OUT * (size_t)nq * sizeof(float)))
    return -3;
  DevModel M = p->hm;
  M.geom_rbound = (const float*)dr.p;
  if (!dm.in(&M, sizeof M)) return -3;
  const int nblk = blocks_for((nq + chunk - 1) / chunk);
  hipLaunchKernelGGL(k_list_rows, dim3(nblk), dim3(64), 0, 0, (const DevModel*)dm.p, p->n, (const float*)dg.p, nq, chunk, nblk, (float*)dout.p);
  return dout.out(out, PAIR_OUT * (size_t)nq * sizeof(float)) ? 0 : -3;
}

}  // extern "C"
