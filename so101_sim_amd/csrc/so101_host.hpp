// Host layer shared by the two engines' handles (so101_sim of so101_hip.hip, TreeHandle of so101_tree_host.hpp): device guard, HIP error helper, owned
// allocations, streams and events, the prefetch's side stream, the env slices' streams, the loader of a blob's collision geometry, cameras, tool calls.
// The general-tree engine is compiled twice (tu_tree.hip inside tv32 / tv64) and the emulator build of the tests includes every .hip
// into one translation unit: everything here is inline, outside those namespaces, and depends on no T* macro.
#pragma once
#include <hip/hip_runtime.h>
#include "so101_blob.hpp"
#include "../../include/so101.h"
#include "so101_tables.hpp"
#include "so101_tool_chain.hpp"
#include "so101_contact_report.hpp"
#include "so101_step_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// what every handle carries: its device, the device allocations, streams and events it owns, its last error message
struct HostHandle {
  int device = 0;
  std::vector<void*> owned;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> events;
  std::string err;
};

inline bool hip_ok(HostHandle* s, hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  s->err = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}

// Every entry point that touches HIP runs with the handle's device current and restores the caller's device on exit
// (a handle is bound to one device; its streams, events and allocations belong to it).
struct DeviceGuard {
  int prev = -1, dev;
  bool ok;
  explicit DeviceGuard(HostHandle* s) : dev(s->device) {
    ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess);
    if (!ok) s->err = "hipSetDevice: cannot make the handle's device current";
  }
  ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};
#define GUARD_DEVICE(s) DeviceGuard guard_(s); if (!guard_.ok) return SO101_ERR_HIP

// `count` elements (at least one) owned by the handle, every byte set to `fill` (fill < 0: left as hipMalloc returns them)
template <typename T>
bool dev_alloc(HostHandle* s, T** out, size_t count, int fill, const char* what) {
  void* p = nullptr;
  size_t bytes = sizeof(T) * (count ? count : 1);
  if (!hip_ok(s, hipMalloc(&p, bytes), what)) return false;
  s->owned.push_back(p);
  if (fill >= 0 && !hip_ok(s, hipMemset(p, fill, bytes), what)) return false;
  *out = (T*)p;
  return true;
}

// device copy of a host array / of one struct, owned by the handle
template <typename T>
bool upload(HostHandle* s, const std::vector<T>& v, const T** out) {
  T* p = nullptr;
  if (!dev_alloc(s, &p, v.size(), -1, "hipMalloc(model)")) return false;
  if (!v.empty() && !hip_ok(s, hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy(model)")) return false;
  *out = p;
  return true;
}
template <typename T>
bool upload_one(HostHandle* s, const T& v, T** out) {
  return dev_alloc(s, out, 1, -1, "hipMalloc(model)") && hip_ok(s, hipMemcpy(*out, &v, sizeof(T), hipMemcpyHostToDevice), "hipMemcpy(model)");
}

// a non-blocking stream owned by the handle (prioritised: created at `priority` of hipDeviceGetStreamPriorityRange); an event without timing
inline bool new_stream(HostHandle* s, hipStream_t* out, bool prioritised = false, int priority = 0) {
  bool ok = prioritised ? hip_ok(s, hipStreamCreateWithPriority(out, hipStreamNonBlocking, priority), "hipStreamCreateWithPriority")
                        : hip_ok(s, hipStreamCreateWithFlags(out, hipStreamNonBlocking), "hipStreamCreate");
  if (ok) s->streams.push_back(*out);
  return ok;
}
inline bool new_event(HostHandle* s, hipEvent_t* out) {
  if (!hip_ok(s, hipEventCreateWithFlags(out, hipEventDisableTiming), "hipEventCreate")) return false;
  s->events.push_back(*out);
  return true;
}

// everything the handle owns: the streams drained first, so nothing of them still runs on memory that is about to go
inline void free_owned(HostHandle* s) {
  for (hipStream_t st : s->streams) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  for (hipEvent_t ev : s->events) (void)hipEventDestroy(ev);
  for (void* p : s->owned) (void)hipFree(p);
  s->streams.clear(); s->events.clear(); s->owned.clear();
}

// The side stream of a reset prefetch: one launch at a time on the lowest-priority stream, behind whatever the caller's stream held when it was enqueued:
// `if (side.begin(st)) { <launches on side.stream>; side.launched(); }`.  begin() is false while the previous launch still runs (the next one refills).
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr, main_ev = nullptr;
  bool pending = false;
  bool setup(HostHandle* s) {
    int lo = 0, hi = 0;
    return hip_ok(s, hipDeviceGetStreamPriorityRange(&lo, &hi), "hipDeviceGetStreamPriorityRange") && new_stream(s, &stream, true, lo) &&
           new_event(s, &done) && new_event(s, &main_ev);
  }
  bool begin(hipStream_t caller) {
    if (pending && hipEventQuery(done) != hipSuccess) { (void)hipGetLastError(); return false; }      // (not ready is a status, not an error to keep)
    pending = false;
    return hipEventRecord(main_ev, caller) == hipSuccess && hipStreamWaitEvent(stream, main_ev, 0) == hipSuccess;
  }
  void launched() { if (hipEventRecord(done, stream) == hipSuccess) pending = true; }
  bool drain(HostHandle* s, const char* what) {
    pending = false;
    return !stream || hip_ok(s, hipStreamSynchronize(stream), what);
  }
};

// Env slices whose launch chains overlap, each on a stream of its own: fork(caller, n) once, then per lane g its chain on stream_of(g) and
// join(g).  One lane runs on the caller's stream and touches no event.
template <int MAX>
struct StreamLanes {
  hipStream_t stream[MAX] = {}, caller = nullptr;
  hipEvent_t done[MAX] = {}, begin = nullptr;
  int n = 1;
  bool setup(HostHandle* s, const int* priority = nullptr) {      // priority: [MAX] stream priorities, NULL for plain streams
    for (int g = 0; g < MAX; g++)
      if (!new_stream(s, &stream[g], priority != nullptr, priority ? priority[g] : 0) || !new_event(s, &done[g])) return false;
    return new_event(s, &begin);
  }
  bool fork(HostHandle* s, hipStream_t from, int lanes) {
    caller = from; n = lanes;
    return n == 1 || hip_ok(s, hipEventRecord(begin, caller), "hipEventRecord");
  }
  bool stream_of(HostHandle* s, int g, hipStream_t* out) {         // lane g's stream, behind what the caller's held at the fork
    *out = n == 1 ? caller : stream[g];
    return n == 1 || hip_ok(s, hipStreamWaitEvent(*out, begin, 0), "hipStreamWaitEvent");
  }
  bool join(HostHandle* s, int g) {
    return n == 1 || (hip_ok(s, hipEventRecord(done[g], stream[g]), "hipEventRecord") && hip_ok(s, hipStreamWaitEvent(caller, done[g], 0), "hipStreamWaitEvent"));
  }
};

inline void h_quat2mat(float* m, const float* q) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = 1 - 2 * (y * y + z * z); m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = 1 - 2 * (x * x + z * z); m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = 1 - 2 * (x * x + y * y);
}

// ---------------------------------------------------------------------------------------------------- geometry of a model blob
// The geom_* / mesh_vert / pair_geom entries of a blob whose scalars ngeom, npair and nvert exist (the engines check their scalars first):
// every array the loader and the engines index is there with the length they rely on, geom_body and pair_geom are in range, vertex ranges
// lie inside mesh_vert.  ngeom_max: the engine's ceiling (at most 256: a packed pair word carries a geom in 8 bits).  A stale or foreign
// blob is rejected here instead of being dereferenced; false with the message in `err`.
inline bool check_geometry(const BlobView& b, size_t nbody, size_t ngeom_max, std::string& err) {
  auto fail = [&](const std::string& msg) { err = msg; return false; };
  size_t ng = (size_t)b.I("ngeom")[0], np = (size_t)b.I("npair")[0], nvert = (size_t)b.I("nvert")[0];
  if (ng > ngeom_max) return fail("too many collision geoms for this build");
  if (np > (1u << 24) || nvert > (1u << 24)) return fail("blob dimensions out of range");
  struct Need { const char* name; size_t count; };
  const Need arrays[] = {
    {"geom_type", ng}, {"geom_body", ng}, {"geom_condim", ng}, {"geom_vertadr", ng}, {"geom_vertnum", ng}, {"geom_pos", 3 * ng}, {"geom_quat", 4 * ng},
    {"geom_size", 3 * ng}, {"geom_friction", 3 * ng}, {"geom_solref", 2 * ng}, {"geom_solimp", 5 * ng}, {"geom_center", 3 * ng}, {"geom_aabb", 6 * ng},
    {"geom_solmix", ng}, {"geom_margin", ng}, {"geom_gap", ng}, {"geom_priority", ng}, {"geom_rbound", ng}, {"mesh_vert", 3 * nvert}, {"pair_geom", 2 * np}};
  for (const Need& a : arrays) if (b.count(a.name) < a.count) return fail(std::string("blob entry missing or too short: ") + a.name);
  for (int v : b.I("geom_body")) if (v < 0 || (size_t)v >= nbody) return fail("blob index array out of range");
  for (int v : b.I("pair_geom")) if (v < 0 || (size_t)v >= ng) return fail("blob index array out of range");
  auto gva = b.I("geom_vertadr"), gvn = b.I("geom_vertnum"), gty = b.I("geom_type");
  for (size_t g = 0; g < ng; g++) if (gvn[g] > 0 && (gva[g] < 0 || (size_t)gva[g] + (size_t)gvn[g] > nvert)) return fail("geom vertex range outside mesh_vert");
  // (the support tables and every support query of a hull need at least one vertex)
  for (size_t g = 0; g < ng; g++) if (gty[g] == G_MESH && gvn[g] <= 0) return fail("mesh geom without vertices (geom_vertnum <= 0)");
  return true;
}

// Every geometry pointer of M, and ngeom / npair / nvert, from a blob that passed check_geometry().  The engine supplies what differs between
// the two: geom_dyn (SO100: index of the dynamic body or -1; tree: body id) and the geoms' frames geom_pos [g][3] / geom_mat [g][9] (SO100:
// static geoms resolved to the world; tree: body-local).  Built here: the packed pair words, the vertices as struct-of-arrays, the hulls'
// support-bound tables and - support_lists: the SO100 engine's k_narrow reads them, the tree engine does not and keeps hl_entry / hl_off
// NULL - their support-vertex lists (so101_tables.hpp).  SO101_NO_SBT / SO101_NO_HL in the environment (tests and kernel experiments, read at
// every create) leave hull_sbt / hl_entry and hl_off NULL: the oriented-box filter alone, every query scans the whole hull.
// false: a HIP call failed (s->err).
inline bool upload_geometry(HostHandle* s, const BlobView& b, const std::vector<int>& geom_dyn, const std::vector<float>& geom_pos, const std::vector<float>& geom_mat,
                            bool support_lists, DevModel& M) {
  M.ngeom = b.I("ngeom")[0]; M.npair = b.I("npair")[0]; M.nvert = b.I("nvert")[0];
  const int ngeom = M.ngeom, nvert = M.nvert;
  auto gtype = b.I("geom_type"), gva = b.I("geom_vertadr"), gvn = b.I("geom_vertnum"), pairs = b.I("pair_geom");
  auto mv = b.F("mesh_vert");
  std::vector<float> vx(nvert), vy(nvert), vz(nvert);
  for (int i = 0; i < nvert; i++) { vx[i] = mv[3 * i]; vy[i] = mv[3 * i + 1]; vz[i] = mv[3 * i + 2]; }
  // broadphase pair list, one word per pair: geom1 | geom2 << 8 | (geom1 is a plane) << 16, geom types ordered
  std::vector<unsigned int> packed(M.npair);
  for (int k = 0; k < M.npair; k++) {
    int g1 = pairs[2 * k], g2 = pairs[2 * k + 1];
    if (gtype[g1] > gtype[g2]) std::swap(g1, g2);
    packed[k] = (unsigned int)g1 | ((unsigned int)g2 << 8) | ((gtype[g1] == G_PLANE ? 1u : 0u) << 16);
  }
  // support-bound tables of the hulls (so101_model.hpp DevModel::hull_sbt; obb_filter and the tree's broadphase)
  M.hull_sbt = nullptr;
  if (!getenv("SO101_NO_SBT")) {
    std::vector<float> sbt((size_t)ngeom * SBT_DIM, 0.f);
    for (int g = 0; g < ngeom; g++)
      if (gtype[g] == G_MESH) build_support_bounds(&mv[3 * (size_t)gva[g]], gvn[g], &sbt[(size_t)g * SBT_DIM]);
    if (!upload(s, sbt, &M.hull_sbt)) return false;
  }
  // support-vertex lists (so101_model.hpp DevModel::hl_entry): per hull and cube-map cell the vertices that can win a support query there
  M.hl_entry = nullptr; M.hl_off = nullptr;
  if (support_lists && !getenv("SO101_NO_HL")) {
    std::vector<float> hle; std::vector<unsigned int> hlo((size_t)ngeom * (HL_CELLS + 1), 0u);
    for (int g = 0; g < ngeom; g++) {
      unsigned int* off = &hlo[(size_t)g * (HL_CELLS + 1)];
      if (gtype[g] != G_MESH) { for (int c = 0; c <= HL_CELLS; c++) off[c] = (unsigned int)(hle.size() / 4); continue; }
      build_support_lists(&mv[3 * (size_t)gva[g]], gvn[g], hle, off);
    }
    if (!(upload(s, hle, &M.hl_entry) && upload(s, hlo, &M.hl_off))) return false;
  }
  return upload(s, gtype, &M.geom_type) && upload(s, geom_dyn, &M.geom_dyn) && upload(s, b.I("geom_condim"), &M.geom_condim) &&
         upload(s, gva, &M.geom_vertadr) && upload(s, gvn, &M.geom_vertnum) && upload(s, geom_pos, &M.geom_pos) && upload(s, geom_mat, &M.geom_mat) &&
         upload(s, b.F("geom_size"), &M.geom_size) && upload(s, b.F("geom_friction"), &M.geom_friction) && upload(s, b.F("geom_solref"), &M.geom_solref) &&
         upload(s, b.F("geom_solimp"), &M.geom_solimp) && upload(s, b.F("geom_center"), &M.geom_center) && upload(s, b.F("geom_aabb"), &M.geom_aabb) &&
         upload(s, b.F("geom_rbound"), &M.geom_rbound) && upload(s, vx, &M.vx) && upload(s, vy, &M.vy) && upload(s, vz, &M.vz) &&
         upload(s, pairs, &M.pair) && upload(s, packed, &M.pair_packed);
}

// ---------------------------------------------------------------------------------------------------- depth / segmentation cameras
// What both handles keep for so101_set_hull_planes / so101_render and their so101_tree_* twins: host copies of what the plane check reads, the
// uploaded planes, the frames scratch of the render calls.
struct RenderHost {
  std::vector<int> gtype, vertadr, vertnum;
  std::vector<float> vert;                 // [nvert][3]
  float* hull_planes = nullptr;            // device [n][4] unit outward normal, offset: n . x + d <= 0 inside (geom frame)
  int* plane_adr = nullptr;                // device [ngeom + 1]
  bool planes_set = false;
  float *frames = nullptr, *cams = nullptr;      // device [cap][ngeom][RENDER_FRAME], [cap][RENDER_MAXCAM][RENDER_CAMFRAME]
  size_t cap = 0;
  float* px_depth = nullptr; int* px_seg = nullptr;      // device [px_cap] each: depth / seg of a colour render whose caller asked for neither
  size_t px_cap = 0;
  int ngeom = 0;
  void load(const BlobView& b) { ngeom = b.I("ngeom")[0]; gtype = b.I("geom_type"); vertadr = b.I("geom_vertadr"); vertnum = b.I("geom_vertnum"); vert = b.F("mesh_vert"); }
  bool has_meshes() const { for (int t : gtype) if (t == G_MESH) return true; return false; }
  // device bytes of the planes of an upload / of the frames scratch per rendered env (SO101_INFO_SCRATCH_BYTES counts them)
  size_t plane_bytes(size_t n) const { return sizeof(float) * 4 * (n ? n : 1) + sizeof(int) * ((size_t)ngeom + 1); }
  size_t frame_bytes() const { return sizeof(float) * ((size_t)ngeom * RENDER_FRAME + RENDER_MAXCAM * RENDER_CAMFRAME); }

  // planes that passed check_hull_planes() become the tables of the next render (a render in flight reads the old ones: they stay allocated
  // until the handle goes); false: a HIP call failed (s->err)
  bool upload_planes(HostHandle* s, const float* planes, const int32_t* adr) {
    const size_t n = (size_t)adr[ngeom];
    float* dp = nullptr; int* da = nullptr;
    if (!dev_alloc(s, &dp, 4 * n, -1, "hipMalloc(hull planes)") || !dev_alloc(s, &da, (size_t)ngeom + 1, -1, "hipMalloc(hull planes)")) return false;
    if (n && !hip_ok(s, hipMemcpy(dp, planes, sizeof(float) * 4 * n, hipMemcpyHostToDevice), "hipMemcpy(hull planes)")) return false;
    if (!hip_ok(s, hipMemcpy(da, adr, sizeof(int) * ((size_t)ngeom + 1), hipMemcpyHostToDevice), "hipMemcpy(hull planes)")) return false;
    hull_planes = dp; plane_adr = da; planes_set = true;
    return true;
  }
  // frames scratch for n_render envs.  Grown outside any stream order: hipFree waits for the device, so a render still reading the old scratch
  // finishes first
  bool reserve(HostHandle* s, size_t n_render) {
    if (n_render <= cap) return true;
    for (void* p : {(void*)frames, (void*)cams}) {
      auto it = std::find(s->owned.begin(), s->owned.end(), p);
      if (p && it != s->owned.end()) { s->owned.erase(it); (void)hipFree(p); }
    }
    frames = nullptr; cams = nullptr; cap = 0;
    if (!dev_alloc(s, &frames, n_render * ngeom * RENDER_FRAME, -1, "hipMalloc(render)") ||
        !dev_alloc(s, &cams, n_render * RENDER_MAXCAM * RENDER_CAMFRAME, -1, "hipMalloc(render)")) return false;
    cap = n_render;
    return true;
  }
  // pixel scratch of the colour renders (so101_render_color / so101_tree_render_color): k_shade reads the depth and seg k_render wrote, so a
  // caller who asks for neither gets them here.  Grown like the frames scratch; 8 bytes per pixel (SO101_INFO_SCRATCH_BYTES counts them)
  size_t pixel_bytes() const { return (sizeof(float) + sizeof(int)) * px_cap; }
  bool reserve_pixels(HostHandle* s, size_t npx) {
    if (npx <= px_cap) return true;
    for (void* p : {(void*)px_depth, (void*)px_seg}) {
      auto it = std::find(s->owned.begin(), s->owned.end(), p);
      if (p && it != s->owned.end()) { s->owned.erase(it); (void)hipFree(p); }
    }
    px_depth = nullptr; px_seg = nullptr; px_cap = 0;
    if (!dev_alloc(s, &px_depth, npx, -1, "hipMalloc(render)") || !dev_alloc(s, &px_seg, npx, -1, "hipMalloc(render)")) return false;
    px_cap = npx;
    return true;
  }
};

// The contract of so101_set_hull_planes (include/so101.h) on HOST arrays, before anything is uploaded: non-mesh geoms have empty ranges, a mesh
// geom has at least 4 planes, | |n| - 1 | <= 1e-4, every vertex of the hull has n . v + d <= 1e-5, every plane has a vertex within 1e-5 of it.
// false with "<api>: geom <g>: <what>" in s->err.
inline bool check_hull_planes(HostHandle* s, const char* api, const RenderHost& R, const float* planes, const int32_t* plane_adr) {
  const int ng = (int)R.gtype.size();
  auto fail = [&](int g, const std::string& what) { s->err = std::string(api) + ": geom " + std::to_string(g) + ": " + what; return false; };
  if (plane_adr[0] != 0) return fail(0, "plane_adr must start at 0");
  for (int g = 0; g < ng; g++) {
    const int k0 = plane_adr[g], k1 = plane_adr[g + 1];
    if (k1 < k0 || k1 > (1 << 24)) return fail(g, "plane range is not ascending");
    if (R.gtype[g] != G_MESH) { if (k1 != k0) return fail(g, "not a mesh geom, its plane range must be empty"); continue; }
    if (k1 - k0 < 4) return fail(g, "a mesh geom needs at least 4 planes");
    const float* v = &R.vert[3 * (size_t)R.vertadr[g]];
    const int nv = R.vertnum[g];
    for (int k = k0; k < k1; k++) {
      const double nx = planes[4 * (size_t)k], ny = planes[4 * (size_t)k + 1], nz = planes[4 * (size_t)k + 2], d = planes[4 * (size_t)k + 3];
      const double len = std::sqrt(nx * nx + ny * ny + nz * nz);
      if (!(std::fabs(len - 1.0) <= 1e-4)) return fail(g, "plane " + std::to_string(k - k0) + " has no unit normal");
      double top = -1e30;
      for (int i = 0; i < nv; i++) top = std::max(top, nx * v[3 * i] + ny * v[3 * i + 1] + nz * v[3 * i + 2] + d);
      if (!(top <= 1e-5)) return fail(g, "plane " + std::to_string(k - k0) + " cuts off a hull vertex");
      if (!(top >= -1e-5)) return fail(g, "plane " + std::to_string(k - k0) + " touches no hull vertex");
    }
  }
  return true;
}

// The arguments of a render call that no engine reads differently: counts, sizes, the tile count, and the cameras into the kernel argument
// (pixel scale 2 tan(fovy / 2) / H in double).  body_max: the highest body a camera may be fixed to.  false (SO101_ERR_ARG) with s->err set.
inline bool render_arguments(HostHandle* s, const char* api, const so101_camera* cams, int ncam, int height, int width, int n_render, int n_envs,
                             bool has_index, bool has_output, int body_max, RenderCams& rc) {
  const std::string a(api);
  if (!cams || ncam < 1 || ncam > RENDER_MAXCAM || height < 1 || height > 4096 || width < 1 || width > 4096 || n_render < 1 || !has_output) {
    s->err = a + ": bad argument (1 <= ncam <= 8, 1 <= height, width <= 4096, n_render >= 1, depth or seg)"; return false;
  }
  if (!has_index && n_render > n_envs) { s->err = a + ": n_render exceeds the envs of the handle"; return false; }
  const unsigned long long blocks = (unsigned long long)n_render * ncam * ((height + 7) / 8) * ((width + 7) / 8);
  if (blocks > 0x7fffffffull) { s->err = a + ": more than 2^31 - 1 pixel tiles in one call"; return false; }
  for (int k = 0; k < ncam; k++) {
    if (cams[k].body < -1 || cams[k].body > body_max || !(cams[k].fovy_deg > 0.f && cams[k].fovy_deg < 180.f)) {
      s->err = a + ": camera " + std::to_string(k) + ": body must be -1 .. " + std::to_string(body_max) + " and 0 < fovy_deg < 180"; return false;
    }
    rc.cam[k].body = cams[k].body;
    rc.cam[k].scale = (float)(2.0 * std::tan(0.5 * (double)cams[k].fovy_deg * 3.14159265358979323846 / 180.0) / (double)height);
    memcpy(rc.cam[k].pos, cams[k].pos, sizeof rc.cam[k].pos); memcpy(rc.cam[k].mat, cams[k].mat, sizeof rc.cam[k].mat);
  }
  return true;
}

// The arguments of a colour render beyond those of render_arguments(): the shading into the kernel argument.  false (SO101_ERR_ARG) with s->err set.
inline bool shade_arguments(HostHandle* s, const char* api, const so101_shading* shading, const float* geom_rgb, const so101_color_out* out, ShadeParams& S) {
  const std::string a(api);
  if (!shading) { s->err = a + ": NULL shading"; return false; }
  if (!geom_rgb) { s->err = a + ": NULL geom_rgb"; return false; }
  if (!out) { s->err = a + ": NULL out"; return false; }
  if (!out->rgb && !out->normal && !out->depth && !out->seg) { s->err = a + ": no output pointer at all"; return false; }
  if (shading->nlight < 0 || shading->nlight > SO101_MAX_LIGHTS) { s->err = a + ": nlight must be 0 .. " + std::to_string(SO101_MAX_LIGHTS); return false; }
  auto colour = [](const float* v) { for (int k = 0; k < 3; k++) if (!(std::isfinite(v[k]) && v[k] >= 0.f)) return false; return true; };
  if (!colour(shading->ambient)) { s->err = a + ": ambient must be finite and >= 0"; return false; }
  if (!colour(shading->background)) { s->err = a + ": background must be finite and >= 0"; return false; }
  S = ShadeParams{};
  memcpy(S.ambient, shading->ambient, sizeof S.ambient); memcpy(S.background, shading->background, sizeof S.background);
  S.nlight = shading->nlight;
  for (int l = 0; l < shading->nlight; l++) {
    const auto& L = shading->light[l];
    if (!colour(L.diffuse)) { s->err = a + ": light " + std::to_string(l) + ": diffuse must be finite and >= 0"; return false; }
    if (!L.headlight) {
      const double len = std::sqrt((double)L.dir[0] * L.dir[0] + (double)L.dir[1] * L.dir[1] + (double)L.dir[2] * L.dir[2]);
      if (!(std::fabs(len - 1.0) <= 1e-4)) { s->err = a + ": light " + std::to_string(l) + ": dir is no unit vector (| |dir| - 1 | > 1e-4)"; return false; }
      memcpy(S.dir[l], L.dir, sizeof S.dir[l]);
    }
    memcpy(S.diffuse[l], L.diffuse, sizeof S.diffuse[l]);
    S.headlight[l] = L.headlight != 0;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------- Cartesian tool control
// What the tool calls of both engines check before they build their chain and launch (so101_tool_chain.hpp).  Each returns SO101_OK or the
// status to return with "<api>: <what>" in s->err.  Tool: so101_tool / so101_tree_tool; Cfg: so101_ik_config / so101_tree_ik_config.

// the tool is there, its frame finite and orthonormal (the body is the engine's to check)
template <typename Tool>
int check_tool_frame(HostHandle* s, const char* api, const Tool* tool) {
  const std::string a(api);
  if (!tool) { s->err = a + ": NULL tool"; return SO101_ERR_ARG; }
  for (int i = 0; i < 3; i++) if (!std::isfinite(tool->pos[i])) { s->err = a + ": tool pos is not finite"; return SO101_ERR_ARG; }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double d = 0.0;
      for (int k = 0; k < 3; k++) d += (double)tool->mat[3 * k + i] * (double)tool->mat[3 * k + j];
      if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-4)) { s->err = a + ": tool mat is not orthonormal (|M^T M - I| > 1e-4)"; return SO101_ERR_ARG; }
    }
  return SO101_OK;
}

// the count and where the joints come from: explicit values (has_q) or the handle's bound state, all of it or the envs of env_index
inline int check_tool_entries(HostHandle* s, const char* api, bool has_q, bool has_index, int n, bool bound, int n_envs) {
  const std::string a(api);
  if (n < 1 || n > (1 << 26)) { s->err = a + ": n must be 1 .. 2^26"; return SO101_ERR_ARG; }      // (the kernels index entries with int)
  if (has_q && has_index) { s->err = a + ": env_index selects envs of the bound state, it cannot be combined with explicit joint values"; return SO101_ERR_ARG; }
  if (!has_q) {
    if (!bound) { s->err = a + ": state buffers not bound (bind the state first, or pass the joint values)"; return SO101_ERR_STATE; }
    if (!has_index && n > n_envs) { s->err = a + ": n exceeds the envs of the handle"; return SO101_ERR_ARG; }
  }
  return SO101_OK;
}

// the settings every default config starts from (include/so101.h); the limits - and the tree engine's free_mask - are the engine's to add
template <typename Cfg>
void ik_default_settings(Cfg* cfg) {
  memset(cfg, 0, sizeof *cfg);
  cfg->mode = 1; cfg->max_iters = 60; cfg->tol_pos = 1e-4f; cfg->tol_rot = 1e-3f; cfg->rot_weight = 0.1f; cfg->damping = 1e-6f; cfg->max_step = 0.5f;
}

// the fields of a config and the arrays an IK call cannot do without, checked over the nio columns the call reads, into the kernel argument
template <int NC, typename Cfg>
int ik_settings(HostHandle* s, const char* api, const Cfg* cfg, int nio, unsigned int free_mask, bool has_target_pos, bool has_target_mat, bool has_q_out,
                IkSettings<NC>& C) {
  auto bad = [&](const char* msg) { s->err = std::string(api) + ": " + msg; return (int)SO101_ERR_ARG; };
  if (!cfg) return bad("NULL config");
  if (!has_target_pos || !has_q_out) return bad("target_pos and q_out are required");
  if (cfg->mode < 0 || cfg->mode > 2) return bad("mode must be 0, 1 or 2");
  if (cfg->max_iters < 0 || cfg->max_iters > 1000) return bad("max_iters must be 0 .. 1000");
  if (!(cfg->tol_pos > 0.f) || !(cfg->tol_rot > 0.f) || !(cfg->rot_weight > 0.f) || !(cfg->max_step > 0.f)) return bad("tol_pos, tol_rot, rot_weight and max_step must be positive");
  if (!(cfg->damping >= 0.f)) return bad("damping must not be negative");
  for (int k = 0; k < nio; k++) if (!(cfg->q_lo[k] <= cfg->q_hi[k])) return bad("q_lo must not exceed q_hi");
  if (nio < 32 && (free_mask >> nio) != 0u) return bad("free_mask has bits at or above the number of columns of the chain");
  if (cfg->mode != 0 && !has_target_mat) return bad("modes 1 and 2 need target_mat");
  C = IkSettings<NC>{};
  C.mode = cfg->mode; C.max_iters = cfg->max_iters; C.tol_pos = cfg->tol_pos; C.tol_rot = cfg->tol_rot; C.rot_weight = cfg->rot_weight;
  C.damping = cfg->damping; C.max_step = cfg->max_step; C.free_mask = free_mask;
  for (int k = 0; k < nio; k++) { C.q_lo[k] = cfg->q_lo[k]; C.q_hi[k] = cfg->q_hi[k]; }
  return SO101_OK;
}

// ---------------------------------------------------------------------------------------------------- contact sensing
// What so101_contacts and so101_tree_contacts check before they launch (k_contacts of so101_contacts.hpp, k_tree_contacts of so101_tree_kernels.hpp),
// in the order their header comment lists it, and how they pack the kernel arguments of the shared report (so101_contact_report.hpp).  Each check
// returns SO101_OK or SO101_ERR_ARG with "<api>: <what>" in s->err.

// the outputs, the count and the pair arguments (the groups themselves: check_contact_group)
inline int check_contact_arguments(HostHandle* s, const char* api, const so101_contact_out* o, bool has_index, int n, int n_envs, int forces, bool has_pairs, int npair) {
  const char* bad = nullptr;
  if (!o) bad = "NULL out";
  else if (!o->count && !o->flags && !o->geom && !o->dist && !o->pos && !o->frame && !o->force && !o->pair_count && !o->pair_dist && !o->pair_normal && !o->pair_force)
    bad = "no output (every pointer of out is NULL)";
  else if (n < 1 || n > (1 << 26)) bad = "n must be 1 .. 2^26";
  else if (!has_index && n > n_envs) bad = "n exceeds the envs of the handle";
  else if (npair < 0 || npair > SO101_TOUCH_MAX_PAIRS) bad = "npair must be 0 .. 16";
  else if (npair > 0 && !has_pairs) bad = "NULL pairs with npair > 0";
  else if (npair == 0 && (o->pair_count || o->pair_dist || o->pair_normal || o->pair_force)) bad = "a pair output with npair == 0";
  else if (!forces && (o->force || o->pair_normal || o->pair_force)) bad = "force, pair_normal and pair_force need forces != 0";
  if (bad) { s->err = std::string(api) + ": " + bad; return SO101_ERR_ARG; }
  return SO101_OK;
}

// the same for so101_proximity and so101_tree_proximity: the outputs, the count and the pair arguments
inline int check_proximity_arguments(HostHandle* s, const char* api, const so101_proximity_out* o, bool has_index, int n, int n_envs, bool has_pairs, int npair) {
  const char* bad = nullptr;
  if (!o) bad = "NULL out";
  else if (!o->dist && !o->geom && !o->point && !o->normal && !o->flags && !o->queries) bad = "no output (every pointer of out is NULL)";
  else if (n < 1 || n > (1 << 26)) bad = "n must be 1 .. 2^26";
  else if (!has_index && n > n_envs) bad = "n exceeds the envs of the handle";
  else if (npair < 1 || npair > SO101_TOUCH_MAX_PAIRS) bad = "npair must be 1 .. 16";
  else if (!has_pairs) bad = "NULL pairs";
  if (bad) { s->err = std::string(api) + ": " + bad; return SO101_ERR_ARG; }
  return SO101_OK;
}

// one group of pair p (side 0: a, 1: b), `nword` 32-bit words: not empty, no bit at or beyond ngeom
inline int check_contact_group(HostHandle* s, const char* api, const uint32_t* w, int nword, int p, int side, int ngeom) {
  bool any = false;
  for (int g = 0; g < 32 * nword; g++) {
    if (!((w[g >> 5] >> (g & 31)) & 1u)) continue;
    any = true;
    if (g >= ngeom) {
      s->err = std::string(api) + ": pair " + std::to_string(p) + ", group " + (side ? "b" : "a") + ": bit " + std::to_string(g) + " is at or beyond ngeom = " + std::to_string(ngeom);
      return SO101_ERR_ARG;
    }
  }
  if (!any) { s->err = std::string(api) + ": pair " + std::to_string(p) + ", group " + (side ? "b" : "a") + " is empty"; return SO101_ERR_ARG; }
  return SO101_OK;
}

// the npair pairs of a call, checked group by group (pair 0 side a, pair 0 side b, pair 1 ...) and packed into the kernel argument
template <int NW, class Pair>
int pack_touch_pairs(HostHandle* s, const char* api, const Pair* pairs, int npair, int ngeom, TouchPairsT<NW>& T) {
  T.npair = npair;
  for (int p = 0; p < npair; p++) {
    for (int side = 0; side < 2; side++) {
      const uint32_t* w = side ? pairs[p].b : pairs[p].a;
      if (int rc = check_contact_group(s, api, w, NW, p, side, ngeom)) return rc;
      memcpy(side ? T.b[p] : T.a[p], w, sizeof T.a[p]);
    }
  }
  return SO101_OK;
}

inline ContactOut contact_out_of(const so101_contact_out* o) {
  return ContactOut{(int*)o->count, (int*)o->flags, (int*)o->geom, o->dist, o->pos, o->frame, o->force, (int*)o->pair_count, o->pair_dist, o->pair_normal, o->pair_force};
}
