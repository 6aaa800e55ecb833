// General-tree engine, host side under the entry points of tu_tree.hip: the handle, the model blob into a TreeModel, the lazily built sets of the
// reset prefetch and of the launch chain, the chain of a tool's body.  Included once per build of the engine, behind so101_tree_kernels.hpp: no include guard.
namespace TREE_NS {
struct TreeHandle : HostHandle {      // (so101_host.hpp: device, owned allocations, streams and events, err)
  int n_envs = 0;
  TreeModel hm{};
  DevModel hg{};
  TreeModel* dm = nullptr;
  DevModel* dg = nullptr;
  TreeBuffers buf{};
  bool bound = false, env_bound = false, has_task = false;
  TreeTask task{};
  TreeEnvBuffers env{};
  TreeStore store{};
  int iterations = 0; float tolerance = 0.f;
  // reset prefetch: second per-env scratch, cache of next-episode states, the side stream (so101_host.hpp)
  float* scratch2 = nullptr;
  float *cq = nullptr, *cv = nullptr, *cw = nullptr; int* cf = nullptr; unsigned int* ctag = nullptr;
  SideStream side;
  bool prefetch = false;
  // launch chain of the control step (so101_tree_config.pipeline): hand-off buffers, allocated when first asked for
  TreePipe pipe{};
  bool pipeline = false;
  static constexpr int MAXSLICES = 4;
  static_assert(MAXSLICES <= STEP_PLAN_MAX_SLICES, "a TreeStepPlan holds STEP_PLAN_MAX_SLICES slices");
  StreamLanes<MAXSLICES> slices;       // env slices whose chains overlap (one's narrowphase beside another's solve)
  RenderHost render;                   // cameras (so101_tree_set_hull_planes / so101_tree_render; so101_host.hpp)
  int plan[4] = {0, 0, 0, 0};          // what the last so101_tree_step that was enqueued whole launched, counted call by call: env slices, kernel launches, memsets, path (0 none yet, 1 single kernel, 2 launch chain)
};

namespace {
thread_local std::string g_tree_error;

int tree_build(TreeHandle* s, const BlobView& b) {
  auto fail = [&](const std::string& msg) { s->err = msg; return (int)SO101_ERR_MODEL; };
  for (const char* n : {"nq", "nv", "nu", "nbody", "ngeom", "narm", "nfree", "npair", "nvert", "neq", "opt_iterations", "opt_mpr_iterations", "opt_cone_elliptic",
                        "opt_timestep", "opt_impratio", "opt_tolerance", "opt_mpr_tolerance", "stat_meaninertia"})
    if (b.count(n) < 1) return fail(std::string("blob entry missing (not a general-tree model?): ") + n);
  TreeModel& M = s->hm;
  M.nq = b.I("nq")[0]; M.nv = b.I("nv")[0]; M.nu = b.I("nu")[0]; M.nbody = b.I("nbody")[0]; M.ngeom = b.I("ngeom")[0];
  M.npair = b.I("npair")[0]; M.njnt = b.I("narm")[0]; M.nfree = b.I("nfree")[0]; M.neq = b.I("neq")[0];
  if (M.nq > TQ || M.nv > TV || M.nu > TU || M.nbody > TB || M.ngeom > TGEOM || M.njnt > TJ || M.neq > TE || M.nq < 0 || M.nv < 0 || M.nbody < 1)
    return fail("model dimensions outside the general-tree builds (32 bodies, 64 dofs, 64 positions, 16 actuators, 256 geoms)");
  size_t nb = M.nbody, ng = M.ngeom, nv = M.nv, nj = M.njnt, nu = M.nu, ne = M.neq;
  struct Need { const char* name; size_t count; };
  const Need arrays[] = {
    {"body_parent", nb}, {"body_jnttype", nb}, {"body_qposadr", nb}, {"body_dofadr", nb}, {"body_pos", 3 * nb}, {"body_quat", 4 * nb}, {"body_ipos", 3 * nb},
    {"body_iquat", 4 * nb}, {"body_mass", nb}, {"body_inertia", 3 * nb}, {"body_invweight0", 2 * nb}, {"arm_body", nj}, {"dof_body", nv}, {"dof_armature", nv},
    {"dof_damping", nv}, {"dof_frictionloss", nv}, {"dof_invweight0", nv}, {"dof_solref", 2 * nj}, {"dof_solimp", 5 * nj}, {"jnt_axis", 3 * nj}, {"jnt_range", 2 * nj},
    {"jnt_limited", nj}, {"jnt_solref", 2 * nj}, {"jnt_solimp", 5 * nj}, {"jnt_actfrclimited", nj}, {"jnt_actfrcrange", 2 * nj}, {"act_dof", nu}, {"act_gain", nu},
    {"act_bias", 3 * nu}, {"act_ctrlrange", 2 * nu}, {"act_forcerange", 2 * nu}, {"act_ctrllimited", nu}, {"act_forcelimited", nu}, {"eq_dof", 2 * ne},
    {"eq_qposadr", 2 * ne}, {"eq_polycoef", 5 * ne}, {"eq_solref", 2 * ne}, {"eq_solimp", 5 * ne}, {"opt_gravity", 3}};
  for (const Need& a : arrays) if (b.count(a.name) < a.count) return fail(std::string("blob entry missing or too short: ") + a.name);
  auto in_range = [&](const char* name, size_t limit) { for (int v : b.I(name)) if (v < 0 || (size_t)v >= limit) return false; return true; };
  if (!in_range("body_parent", nb) || !in_range("arm_body", nb) || !in_range("dof_body", nb) ||
      !in_range("act_dof", nv) || !in_range("eq_dof", nv) || !in_range("eq_qposadr", M.nq)) return fail("blob index array out of range");
  if (!check_geometry(b, nb, TGEOM, s->err)) return SO101_ERR_MODEL;          // (the geom_* / mesh_vert / pair_geom entries: so101_host.hpp)
  for (float v : b.F("geom_margin")) if (v != 0.f) return fail("geom margin must be 0");
  for (float v : b.F("geom_gap")) if (v != 0.f) return fail("geom gap must be 0");

  M.elliptic = b.I("opt_cone_elliptic")[0]; M.iterations = b.I("opt_iterations")[0];
  M.dt = b.F("opt_timestep")[0]; M.impratio = b.F("opt_impratio")[0]; M.tolerance = b.F("opt_tolerance")[0]; M.meaninertia = b.F("stat_meaninertia")[0];
  auto grav = b.F("opt_gravity"); for (int k = 0; k < 3; k++) M.grav[k] = grav[k];
  auto parent = b.I("body_parent"), jt = b.I("body_jnttype"), qadr = b.I("body_qposadr"), dadr = b.I("body_dofadr"), armb = b.I("arm_body");
  auto bpos = b.F("body_pos"), bquat = b.F("body_quat"), ipos = b.F("body_ipos"), iquat = b.F("body_iquat"), mass = b.F("body_mass"), inertia = b.F("body_inertia"),
       invw = b.F("body_invweight0");
  M.maxdepth = 0;
  for (int i = 0; i < M.nbody; i++) {
    if (i > 0 && parent[i] >= i) return fail("bodies must be numbered parents first");
    M.body_parent[i] = parent[i]; M.body_jnttype[i] = jt[i]; M.body_qposadr[i] = qadr[i]; M.body_dofadr[i] = dadr[i]; M.body_jnt[i] = -1;
    M.body_depth[i] = i == 0 ? 0 : M.body_depth[parent[i]] + 1;
    M.body_anc[i] = (i == 0 ? 0u : M.body_anc[parent[i]]) | (1u << i);
    M.body_dofs[i] = i == 0 ? 0ull : M.body_dofs[parent[i]];
    if (M.body_depth[i] > M.maxdepth) M.maxdepth = M.body_depth[i];
    for (int k = 0; k < 3; k++) { M.body_pos[i][k] = bpos[3 * i + k]; M.body_ipos[i][k] = ipos[3 * i + k]; M.body_inertia[i][k] = inertia[3 * i + k]; }
    for (int k = 0; k < 4; k++) { M.body_quat[i][k] = bquat[4 * i + k]; M.body_iquat[i][k] = iquat[4 * i + k]; }
    M.body_mass[i] = mass[i]; M.body_invweight0[i][0] = invw[2 * i]; M.body_invweight0[i][1] = invw[2 * i + 1];
    int ndof = jt[i] == TJ_FREE ? 6 : (jt[i] == TJ_HINGE || jt[i] == TJ_SLIDE ? 1 : 0);
    if (ndof && (dadr[i] < 0 || dadr[i] + ndof > M.nv)) return fail("body dof address out of range");
    if (ndof && (qadr[i] < 0 || qadr[i] + (ndof == 6 ? 7 : 1) > M.nq)) return fail("body qpos address out of range");
    for (int k = 0; k < ndof; k++) M.body_dofs[i] |= 1ull << (dadr[i] + k);
  }
  auto dbody = b.I("dof_body");
  auto arma = b.F("dof_armature"), damp = b.F("dof_damping"), floss = b.F("dof_frictionloss"), dinv = b.F("dof_invweight0"), dsr = b.F("dof_solref"), dsi = b.F("dof_solimp");
  auto jaxis = b.F("jnt_axis"), jrange = b.F("jnt_range"), jsr = b.F("jnt_solref"), jsi = b.F("jnt_solimp"), jfr = b.F("jnt_actfrcrange");
  auto jlim = b.I("jnt_limited"), jfl = b.I("jnt_actfrclimited");
  for (int j = 0; j < M.njnt; j++) {
    int body = armb[j];
    if (jt[body] != TJ_HINGE && jt[body] != TJ_SLIDE) return fail("arm_body entry without a one-dof joint");
    M.jnt_body[j] = body; M.body_jnt[body] = j; M.jnt_limited[j] = jlim[j]; M.jnt_actfrclimited[j] = jfl[j];
    for (int k = 0; k < 3; k++) M.jnt_axis[j][k] = jaxis[3 * j + k];
    for (int k = 0; k < 2; k++) { M.jnt_range[j][k] = jrange[2 * j + k]; M.jnt_solref[j][k] = jsr[2 * j + k]; M.jnt_actfrcrange[j][k] = jfr[2 * j + k]; }
    for (int k = 0; k < 5; k++) M.jnt_solimp[j][k] = jsi[5 * j + k];
  }
  M.nfric = 0; M.any_damping = 0;
  for (int d = 0; d < M.nv; d++) {
    int body = dbody[d];
    M.dof_body[d] = body; M.dof_jnt[d] = M.body_jnt[body];
    M.dof_armature[d] = arma[d]; M.dof_damping[d] = damp[d]; M.dof_frictionloss[d] = floss[d]; M.dof_invweight0[d] = dinv[d];
    if (damp[d] > 0.f) M.any_damping = 1;
    int j = M.dof_jnt[d];
    M.dof_solref[d][0] = j >= 0 ? dsr[2 * j] : 0.02f; M.dof_solref[d][1] = j >= 0 ? dsr[2 * j + 1] : 1.f;
    const float defimp[5] = {0.9f, 0.95f, 0.001f, 0.5f, 2.f};
    for (int k = 0; k < 5; k++) M.dof_solimp[d][k] = j >= 0 ? dsi[5 * j + k] : defimp[k];
    if (floss[d] > 0.f) { if (M.nfric >= TFR) return fail("too many dofs with frictionloss"); M.fric_dof[M.nfric++] = d; }
  }
  auto adof = b.I("act_dof"), acl = b.I("act_ctrllimited"), afl = b.I("act_forcelimited");
  auto again = b.F("act_gain"), abias = b.F("act_bias"), acr = b.F("act_ctrlrange"), afr = b.F("act_forcerange");
  for (int a = 0; a < M.nu; a++) {
    M.act_dof[a] = adof[a]; M.act_ctrllimited[a] = acl[a]; M.act_forcelimited[a] = afl[a]; M.act_gain[a] = again[a];
    int body = dbody[adof[a]];
    if (jt[body] == TJ_FREE) return fail("actuator on a free body");
    M.act_qposadr[a] = qadr[body];
    for (int k = 0; k < 3; k++) M.act_bias[a][k] = abias[3 * a + k];
    for (int k = 0; k < 2; k++) { M.act_ctrlrange[a][k] = acr[2 * a + k]; M.act_forcerange[a][k] = afr[2 * a + k]; }
    for (int a2 = 0; a2 < a; a2++) if (adof[a2] == adof[a]) return fail("two actuators on one dof");
  }
  auto edof = b.I("eq_dof"), eqa = b.I("eq_qposadr");
  auto epc = b.F("eq_polycoef"), esr = b.F("eq_solref"), esi = b.F("eq_solimp");
  for (int e = 0; e < M.neq; e++) {
    for (int k = 0; k < 2; k++) { M.eq_dof[e][k] = edof[2 * e + k]; M.eq_qposadr[e][k] = eqa[2 * e + k]; M.eq_solref[e][k] = esr[2 * e + k]; }
    for (int k = 0; k < 5; k++) { M.eq_polycoef[e][k] = epc[5 * e + k]; M.eq_solimp[e][k] = esi[5 * e + k]; }
  }
  if (M.neq + M.nfric > 32) return fail("too many scalar constraint rows");

  // geometry: the tables the shared narrowphase reads (DevModel), every geom relative to its body
  DevModel& G = s->hg;
  G.iterations = M.iterations; G.mpr_iter = b.I("opt_mpr_iterations")[0];
  G.dt = M.dt; G.mpr_tol = b.F("opt_mpr_tolerance")[0]; G.impratio = M.impratio; G.tolerance = M.tolerance; G.meaninertia = M.meaninertia;
  auto gquat = b.F("geom_quat");
  std::vector<float> gmat(9 * ng);
  for (size_t g = 0; g < ng; g++) h_quat2mat(&gmat[9 * g], &gquat[4 * g]);
  // (geom_dyn = the body id; no support-vertex lists: k_tree_narrow scans the staged hulls)
  bool ok = upload_geometry(s, b, b.I("geom_body"), b.F("geom_pos"), gmat, false, G) && upload(s, b.I("geom_body"), &M.geom_body) &&
            upload(s, b.F("geom_solmix"), &M.geom_solmix) && upload(s, b.I("geom_priority"), &M.geom_priority);
  M.geom_class = nullptr;
  if (ok && b.count("task_geom_class") >= ng) ok = upload(s, b.I("task_geom_class"), &M.geom_class);
  if (!ok) return SO101_ERR_HIP;
  // task layer (hand-over scenes): absent from the bare-arm blob
  TreeTask& T = s->task;
  T.n_substeps = 10; T.last_step = 1 << 30; T.settle_max = 1000; T.terminate_on_success = 1;
  s->has_task = b.count("task_object_body") >= 1 && b.I("task_object_body")[0] > 0 && b.count("task_obs_qposadr") >= 1;
  if (s->has_task) {
    size_t nbox = b.count("task_nbox") ? (size_t)b.I("task_nbox")[0] : 99;
    size_t npos = b.count("task_obs_qposadr");
    const Need tneed[] = {{"task_container_body", 1}, {"task_box_pos", 3 * nbox}, {"task_box_half", 3 * nbox}, {"task_obj_pos_lo", 3}, {"task_obj_pos_hi", 3},
                          {"task_obj_yaw", 2}, {"task_con_pos_lo", 3}, {"task_con_pos_hi", 3}, {"task_home_ctrl", nu}, {"task_home_qpos", nj},
                          {"task_obs_is_gripper", npos}, {"task_act_is_gripper", nu}, {"task_gripper_limits", 6}, {"body_bvh_aabb", 6 * nb}};
    if (nbox > 2 || npos > TU || npos > 64) return fail("task dimensions out of range");
    for (const Need& a : tneed) if (b.count(a.name) < a.count) return fail(std::string("blob entry missing or too short: ") + a.name);
    T.obj_body = b.I("task_object_body")[0]; T.con_body = b.I("task_container_body")[0]; T.nbox = (int)nbox;
    T.dist_threshold = b.count("task_dist_threshold") ? b.F("task_dist_threshold")[0] : 0.f;
    if (T.obj_body <= 0 || T.obj_body >= M.nbody || T.con_body <= 0 || T.con_body >= M.nbody || jt[T.obj_body] != TJ_FREE || jt[T.con_body] != TJ_FREE)
      return fail("task bodies must be free bodies");
    T.npos = (int)npos; T.nvel = M.njnt;
    auto oq = b.I("task_obs_qposadr"), og = b.I("task_obs_is_gripper"), ag = b.I("task_act_is_gripper");
    for (int k = 0; k < T.npos; k++) { if (oq[k] < 0 || oq[k] >= M.njnt) return fail("task_obs_qposadr out of range"); T.obs_qposadr[k] = oq[k]; T.obs_is_gripper[k] = og[k]; }
    if (T.npos != M.nu) return fail("one commanded position per actuator expected");
    for (int k = 0; k < M.nu; k++) T.act_is_gripper[k] = ag[k];
    auto gl = b.F("task_gripper_limits"); for (int k = 0; k < 6; k++) T.grip[k] = gl[k];
    auto bp = b.F("task_box_pos"), bh = b.F("task_box_half"), bvh = b.F("body_bvh_aabb");
    for (int k = 0; k < T.nbox; k++) for (int i = 0; i < 3; i++) { T.box_pos[k][i] = bp[3 * k + i]; T.box_half[k][i] = bh[3 * k + i]; }
    for (int i = 0; i < 6; i++) T.obj_bvh[i] = bvh[6 * T.obj_body + i];
    auto lo = b.F("task_obj_pos_lo"), hi = b.F("task_obj_pos_hi"), yaw = b.F("task_obj_yaw"), clo = b.F("task_con_pos_lo"), chi = b.F("task_con_pos_hi");
    for (int i = 0; i < 3; i++) { T.obj_lo[i] = lo[i]; T.obj_hi[i] = hi[i]; T.con_lo[i] = clo[i]; T.con_hi[i] = chi[i]; }
    T.obj_yaw[0] = yaw[0]; T.obj_yaw[1] = yaw[1];
    T.kind = b.count("task_kind") ? b.I("task_kind")[0] : 0;
    if (T.kind == 1) {                          // Dining (tasks/base/dining.py): six props, six regions
      if (b.count("task_prop_bodies") < 6 || b.count("task_region_lo") < 18 || b.count("task_region_hi") < 18) return fail("dining blob: task_prop_bodies / task_region_lo / task_region_hi missing");
      auto pbod = b.I("task_prop_bodies"); auto rlo = b.F("task_region_lo"), rhi = b.F("task_region_hi");
      for (int k = 0; k < 6; k++) {
        if (pbod[k] < 1 || pbod[k] >= M.nbody || jt[pbod[k]] != TJ_FREE) return fail("dining blob: task_prop_bodies must name free bodies");
        T.prop_body[k] = pbod[k];
        for (int i = 0; i < 3; i++) { T.region_lo[k][i] = rlo[3 * k + i]; T.region_hi[k][i] = rhi[3 * k + i]; }
      }
    } else if (T.kind != 0) return fail("unknown task_kind");
    auto hq = b.F("task_home_qpos"), hc = b.F("task_home_ctrl");
    for (int k = 0; k < M.njnt; k++) T.home_qpos[k] = hq[k];
    for (int k = 0; k < M.nu; k++) T.home_ctrl[k] = hc[k];
  }
  if (!upload_one(s, M, &s->dm) || !upload_one(s, G, &s->dg)) return SO101_ERR_HIP;
  s->render.load(b);
  return SO101_OK;
}
}  // namespace

static TreeTask task_now(TreeHandle* s) { TreeTask T = s->task; T.n_envs = s->n_envs; T.iterations = s->iterations; T.tolerance = s->tolerance; return T; }
// the store the kernels see: the caller's settled-state tables plus, with the prefetch on, the library's cache of next-episode states
static TreeStore store_now(TreeHandle* s) {
  TreeStore S = s->store;
  S.cq = S.cv = S.cw = nullptr; S.cf = nullptr; S.ctag = nullptr;
  if (s->prefetch && s->ctag) { S.cq = s->cq; S.cv = s->cv; S.cw = s->cw; S.cf = s->cf; S.ctag = s->ctag; }
  return S;
}
static bool tree_prefetch_setup(TreeHandle* s) {          // lazily: second scratch, cache, low-priority stream
  if (s->ctag) return true;
  size_t n = (size_t)s->n_envs;
  const char* what = "hipMalloc(prefetch)";
  return dev_alloc(s, &s->scratch2, n * T_SCRATCH, 0, what) && dev_alloc(s, &s->cq, n * s->hm.nq, 0, what) &&
         dev_alloc(s, &s->cv, n * s->hm.nv, 0, what) && dev_alloc(s, &s->cw, n * s->hm.nv, 0, what) && dev_alloc(s, &s->cf, n, 0, what) &&
         s->side.setup(s) && dev_alloc(s, &s->ctag, n, 0, what);          // (ctag last: it marks the set as complete)
}
static bool tree_pipe_setup(TreeHandle* s) {             // lazily: the hand-off buffers of the launch chain
  if (s->pipe.pose) return true;
  size_t n = (size_t)s->n_envs;
  TreePipe& P = s->pipe;
  float* pose = nullptr;
  const char* what = "hipMalloc(pipeline)";
  bool ok = dev_alloc(s, &P.cand, n * TCAND, 0, what) && dev_alloc(s, &P.ncand, n, 0, what) && dev_alloc(s, &P.rec, n * TCAND * TREC, 0, what) &&
            dev_alloc(s, &P.work, 2 * n * TCAND, 0, what) && dev_alloc(s, &P.counters, (size_t)TreeHandle::MAXSLICES * 2 * TPIPE_MAXSUB, 0, what) && dev_alloc(s, &P.active, n, 0, what) &&
            dev_alloc(s, &P.pflags, n, 0, what) && dev_alloc(s, &P.pdiag, 4 * n, 0, what) && dev_alloc(s, &pose, n * TB * 12, 0, what) && s->slices.setup(s);
  if (ok) P.pose = pose;          // (last: marks the set as complete)
  return ok;
}
// k_tree_prepare with the second scratch on the side stream, behind whatever `stream` holds now (SideStream, so101_host.hpp)
static void launch_tree_prepare(TreeHandle* s, hipStream_t stream) {
  if (!s->prefetch || !s->ctag || s->task.settle_max == 0 || !s->side.begin(stream)) return;
  TreeBuffers B2 = s->buf; B2.scratch = s->scratch2;
  hipLaunchKernelGGL(k_tree_prepare, dim3(s->n_envs), dim3(64), 0, s->side.stream, s->dm, s->dg, task_now(s), B2, (const int*)s->env.episode, store_now(s));
  if (hipGetLastError() == hipSuccess) s->side.launched();
}

// ---- Cartesian tool control (so101_tool_chain.hpp, compiled in tu_misc.hip): the chain of a tool's body, computed per call on the host
// The bodies from the world down to `body` that carry a hinge or slide joint become the columns, root first; the jointless bodies between them are
// folded in double precision into the fixed transform in front of the next joint, what lies below the last joint into the tool's frame (pos, mat
// row-major: identity when `tool` is NULL).  Returns SO101_OK or SO101_ERR_ARG with s->err set; `api` names the caller in the message.
constexpr int TREE_TOOL_MAXCOL = 8;
static_assert(TJ_HINGE == TOOL_HINGE && TJ_SLIDE == TOOL_SLIDE, "the chain's column types are the joint types");
static int tree_tool_chain(TreeHandle* s, const char* api, int body, const so101_tree_tool* tool, ToolChain<TREE_TOOL_MAXCOL>& T, int* dof /* [8] or NULL */) {
  const std::string a(api);
  const TreeModel& M = s->hm;
  if (body < 1 || body >= M.nbody) { s->err = a + ": tool body must be 1 .. nbody - 1 (a body id of the model)"; return SO101_ERR_ARG; }
  int path[TB], np = 0, ncol = 0;
  for (int b = body; b != 0; b = M.body_parent[b]) {
    path[np++] = b;
    if (M.body_jnttype[b] == TJ_FREE) { s->err = a + ": the chain of the tool body contains a free joint (a prop, not an arm link)"; return SO101_ERR_ARG; }
    if (M.body_jnttype[b] == TJ_HINGE || M.body_jnttype[b] == TJ_SLIDE) ncol++;
  }
  if (ncol == 0) { s->err = a + ": the tool body has no joint above it (it is fixed to the world)"; return SO101_ERR_ARG; }
  if (ncol > TREE_TOOL_MAXCOL) { s->err = a + ": the chain of the tool body is longer than 8 joints"; return SO101_ERR_ARG; }
  auto rot = [](const double* q, const double* v, double* o) {          // o = R(q) v
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 3; i++) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
  };
  auto mul = [](const double* p, const double* q, double* o) {
    const double r[4] = {p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                         p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]};
    for (int i = 0; i < 4; i++) o[i] = r[i];
  };
  auto norm = [](double* q) { const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); for (int i = 0; i < 4; i++) q[i] /= n; };
  T = ToolChain<TREE_TOOL_MAXCOL>{};
  T.rquat[0] = 1.f;                           // (the root is the world)
  double P[3] = {0, 0, 0}, Q[4] = {1, 0, 0, 0};
  int k = 0;
  for (int i = np - 1; i >= 0; i--) {
    const int b = path[i];
    double bp[3], bq[4], t[3];
    for (int j = 0; j < 3; j++) bp[j] = M.body_pos[b][j];
    for (int j = 0; j < 4; j++) bq[j] = M.body_quat[b][j];
    norm(bq);
    rot(Q, bp, t);
    for (int j = 0; j < 3; j++) P[j] += t[j];
    mul(Q, bq, Q); norm(Q);
    const int jt = M.body_jnttype[b];
    if (jt == TJ_HINGE || jt == TJ_SLIDE) {
      for (int j = 0; j < 3; j++) { T.pos[k][j] = (float)P[j]; T.axis[k][j] = M.jnt_axis[M.body_jnt[b]][j]; }
      for (int j = 0; j < 4; j++) T.quat[k][j] = (float)Q[j];
      T.type[k] = jt; T.qposadr[k] = M.body_qposadr[b];
      if (dof) dof[k] = M.body_dofadr[b];
      k++;
      P[0] = P[1] = P[2] = 0.0; Q[0] = 1.0; Q[1] = Q[2] = Q[3] = 0.0;
    }
  }
  T.ncol = T.nio = ncol;
  double tp[3] = {0, 0, 0}, tm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, w[3];
  if (tool) { for (int j = 0; j < 3; j++) tp[j] = tool->pos[j]; for (int j = 0; j < 9; j++) tm[j] = tool->mat[j]; }
  rot(Q, tp, w);
  for (int j = 0; j < 3; j++) T.tpos[j] = (float)(P[j] + w[j]);
  for (int c = 0; c < 3; c++) {
    const double col[3] = {tm[c], tm[3 + c], tm[6 + c]};
    rot(Q, col, w);
    for (int r = 0; r < 3; r++) T.tmat[3 * r + c] = (float)w[r];
  }
  return SO101_OK;
}
}  // namespace TREE_NS
