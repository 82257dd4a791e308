// One large fit sharded over the GPUs of a node, entirely inside the library (included by sigp.hip in its anonymous namespace):
// the transports (the library's own RCCL communicator, bound with dlopen; or a caller-supplied one), the panel loop of the
// block-cyclic Cholesky with its look-ahead broadcast, and the sharded triangular solves + fp64 refinement of the fp32 engine.
// A panel is factored by the same primitives as a single-GPU fit (dist_panel / dist_panel_top, sigp_factor.inc).
// Replaces the same statements as the single-GPU path: north/June1st.py:265 (Cholesky), :266-277 (solves, predictions), :246.
//
// Layout.  Panel q = block columns [q W, q W + W_q) (W_q = W except for the last); rank q % world owns it: it alone stores,
// builds and updates those columns (all rows from the panel's diagonal block down, and the 128 ride rows).  Per panel p, in order:
//   owner(p)   applies panel p - 1 to ITS columns first, on its panel stream, then factors the panel there (one in-order latency
//              chain) and packs rows [p W 128, n_pad + 128) x its columns into a contiguous buffer;
//   everyone   takes part in the broadcast of that buffer on the communication stream (RCCL over xGMI) -- ordered after the pack
//              by an event on the owner, and after the last update that read the buffer's previous panel (p - 2) on the others;
//   everyone   updates the panels it owns (q > p) from the buffer on its update stream, behind an event of the broadcast.
// Nothing in the loop waits on the host: no stream synchronisation, no device-to-host read; the pivot info is reduced once at the
// end (MIN over the ranks' first failing pivot).  A host-pointer transport (tests, fabrics without device collectives) stages the
// buffers through pinned memory and synchronises per panel; the arithmetic and its order are the same.

// ---- RCCL, bound at run time -------------------------------------------------------------------------------------------------
// The library is not linked against librccl: a process that never shards a fit does not need it, and a process that already has
// an RCCL (PyTorch-ROCm ships its own next to its own HIP runtime) must get THAT one, not a second copy bound to another runtime.
struct RcclApi {
  void* lib = nullptr;
  std::string path;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclBroadcast) Broadcast = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
};

RcclApi* rccl_api(std::string* why) {
  static std::mutex mu;
  static RcclApi api;
  static bool tried = false;
  static std::string err;
  std::lock_guard<std::mutex> lk(mu);
  if (!tried) {
    tried = true;
    // an RCCL already mapped into the process first (torch's is loaded under the name librccl.so), then the system's
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    for (int pass = 0; pass < 2 && !api.lib; ++pass)
      for (const char* nm : names) {
        if (pass == 0 && nm[0] == '/') continue;
        api.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
        if (api.lib) { api.path = std::string(nm) + (pass == 0 ? " (already loaded in this process)" : ""); break; }
      }
    if (!api.lib) {
      const char* de = dlerror();              // (one call: it clears the message)
      err = std::string("librccl not found (") + (de ? de : "dlopen failed") + ")";
    } else {
      api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
      api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
      api.Broadcast = (decltype(api.Broadcast))dlsym(api.lib, "ncclBroadcast");
      api.AllReduce = (decltype(api.AllReduce))dlsym(api.lib, "ncclAllReduce");
      api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
      api.CommCount = (decltype(api.CommCount))dlsym(api.lib, "ncclCommCount");
      api.CommGetAsyncError = (decltype(api.CommGetAsyncError))dlsym(api.lib, "ncclCommGetAsyncError");
      api.CommAbort = (decltype(api.CommAbort))dlsym(api.lib, "ncclCommAbort");
      api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
      api.Send = (decltype(api.Send))dlsym(api.lib, "ncclSend");
      api.Recv = (decltype(api.Recv))dlsym(api.lib, "ncclRecv");
      api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
      api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
      if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.Broadcast || !api.AllReduce) {
        err = "librccl (" + api.path + ") lacks a required entry point";
        api.lib = nullptr;
      }
    }
  }
  if (!api.lib) { if (why) *why = err; return nullptr; }
  return &api;
}

#define NCCLCHK(h, api, expr)                                                                                   \
  do {                                                                                                          \
    ncclResult_t r_ = (expr);                                                                                   \
    if (r_ != ncclSuccess)                                                                                      \
      return fail(h, SIGP_HIP_ERROR, "%s failed: %s (%s:%d)", #expr, (api)->GetErrorString ? (api)->GetErrorString(r_) : "rccl error", __FILE__, __LINE__); \
  } while (0)

void dist_release(sigp_handle* h) {
  auto& dc = h->dc;
  if (dc.comm) {
    RcclApi* api = rccl_api(nullptr);
    if (api) (void)api->CommDestroy((ncclComm_t)dc.comm);
    dc.comm = nullptr;
  }
  dc.kind = 0; dc.nranks = 1; dc.rank = 0;
  if (dc.s_comm) { (void)hipStreamDestroy(dc.s_comm); dc.s_comm = nullptr; }
  if (dc.hstage) { (void)hipHostFree(dc.hstage); dc.hstage = nullptr; dc.cap_hstage = 0; }
  for (int k = 0; k < 2; ++k) {
    if (dc.pbuf[k]) { (void)hipFree(dc.pbuf[k]); dc.pbuf[k] = nullptr; }
    if (dc.sbuf[k]) { (void)hipFree(dc.sbuf[k]); dc.sbuf[k] = nullptr; }
    if (dc.tbuf[k]) { (void)hipFree(dc.tbuf[k]); dc.tbuf[k] = nullptr; }
    for (hipEvent_t* e : {&dc.ev_pack[k], &dc.ev_bcast[k], &dc.ev_read[k], &dc.ev_first[k], &dc.ev_solve[k], &dc.ev_hot[k]}) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
  }
  dc.cap_pbuf = 0; dc.cap_tbuf = 0;
  if (dc.ev_mark) { (void)hipEventDestroy(dc.ev_mark); dc.ev_mark = nullptr; }
  if (dc.ev_seg) { (void)hipEventDestroy(dc.ev_seg); dc.ev_seg = nullptr; }
  for (auto e : dc.ev_t) (void)hipEventDestroy(e);
  dc.ev_t.clear();
  for (auto e : dc.ev_own) (void)hipEventDestroy(e);
  dc.ev_own.clear();
  for (void** p : {&dc.Uinv, &dc.Vinv, &dc.invP, &dc.ft, &dc.fx, &dc.fr, &dc.fc}) if (*p) { (void)hipFree(*p); *p = nullptr; }
  for (double** p : {&dc.alpha, &dc.pred}) if (*p) { (void)hipFree(*p); *p = nullptr; }
  dc.cap_pred = 0; dc.cap_alpha = 0;
  dc.cap_inv = dc.cap_invP = dc.cap_vec = dc.cap_ft = 0;
  if (dc.dinfo) { (void)hipFree(dc.dinfo); dc.dinfo = nullptr; }
  if (dc.prog) { (void)hipHostFree(dc.prog); dc.prog = nullptr; }
  if (dc.ev_wait) { (void)hipEventDestroy(dc.ev_wait); dc.ev_wait = nullptr; }
  dc.dead = false;
  if (h->dl.mat) { (void)hipFree(h->dl.mat); h->dl.mat = nullptr; h->dl.cap = 0; }
  if (h->dl.dinv) { (void)hipFree(h->dl.dinv); h->dl.dinv = nullptr; h->dl.cap_dinv = 0; }
  h->dl.on = false;
}

int dist_streams(sigp_handle* h) {
  auto& dc = h->dc;
  if (!dc.s_comm) HIPCHK(h, hipStreamCreateWithFlags(&dc.s_comm, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k)
    for (hipEvent_t* e : {&dc.ev_pack[k], &dc.ev_bcast[k], &dc.ev_read[k], &dc.ev_first[k], &dc.ev_solve[k], &dc.ev_hot[k]})
      if (!*e) HIPCHK(h, hipEventCreateWithFlags(e, hipEventDisableTiming));
  if (!dc.ev_mark) HIPCHK(h, hipEventCreateWithFlags(&dc.ev_mark, hipEventDisableTiming));
  if (!dc.ev_seg) HIPCHK(h, hipEventCreateWithFlags(&dc.ev_seg, hipEventDisableTiming));
  if (!dc.dinfo) HIPCHK(h, hipMalloc((void**)&dc.dinfo, 8 * sizeof(double)));
  if (!dc.prog) { HIPCHK(h, hipHostMalloc((void**)&dc.prog, 4 * sizeof(int))); dc.prog[0] = 0; }
  return SIGP_OK;
}

int dist_hstage(sigp_handle* h, size_t bytes) {
  auto& dc = h->dc;
  if (dc.cap_hstage >= bytes) return SIGP_OK;
  if (dc.hstage) HIPCHK(h, hipHostFree(dc.hstage));
  dc.hstage = nullptr; dc.cap_hstage = 0;
  HIPCHK(h, hipHostMalloc(&dc.hstage, bytes));
  dc.cap_hstage = bytes;
  return SIGP_OK;
}

// ---- a dead peer is an error, not a hang ---------------------------------------------------------------------------------------
// Every host-side wait of the sharded path goes through dist_wait: the stream's work is behind an event that is POLLED, with the
// communicator's asynchronous error state (RCCL: ncclCommGetAsyncError) and a deadline (option dist_timeout_ms, default 120 s;
// 0 = wait for ever).  On an error or when the deadline passes the communicator is aborted (ncclCommAbort: its kernels leave the
// streams), the handle's sharded state is marked dead and the call returns SIGP_HIP_ERROR with the panel the update stream had
// reached in sigp_last_error -- the reference's convention is "raise, don't hang" (north/June1st.py:254-256).  A dead handle
// answers every sigp_dist_fit / sigp_dist_predict with the same error until sigp_dist_shutdown (+ a fresh sigp_dist_init*); the
// caller exits non-zero or starts over in a fresh process / handle.
__global__ void progress_kernel(volatile int* word, int value) { *word = value; }

int dist_mark_dead(sigp_handle* h, const char* what, const char* why) {
  auto& dc = h->dc;
  const int reached = dc.prog ? dc.prog[0] : -1;
  if (dc.kind == 1 && dc.comm) {
    RcclApi* api = rccl_api(nullptr);
    if (api && api->CommAbort) (void)api->CommAbort((ncclComm_t)dc.comm);     // kills the communicator's kernels: the library's streams drain
    else if (api) (void)api->CommDestroy((ncclComm_t)dc.comm);
    dc.comm = nullptr;
  }
  dc.dead = true; dc.fit_ok = false; dc.inv_ready = dc.alpha_ready = false;
  h->dl.on = false;
  return fail(h, SIGP_HIP_ERROR, "sharded %s: %s (update stream had reached panel %d of %d; rank %d of %d) -- the communicator is dead: sigp_dist_shutdown, then a fresh "
              "sigp_dist_init / a fresh process", what, why, reached, h->dl.P, dc.rank, dc.nranks);
}

int dist_wait(sigp_handle* h, hipStream_t st, const char* what) {
  auto& dc = h->dc;
  if (dc.kind == 0 || (h->opt_dist_timeout_ms <= 0 && dc.kind != 1)) { HIPCHK(h, hipStreamSynchronize(st)); return SIGP_OK; }
  if (!dc.ev_wait) HIPCHK(h, hipEventCreateWithFlags(&dc.ev_wait, hipEventDisableTiming));
  HIPCHK(h, hipEventRecord(dc.ev_wait, st));
  RcclApi* api = dc.kind == 1 ? rccl_api(nullptr) : nullptr;
  // the deadline measures time WITHOUT progress: it restarts whenever the update stream's panel counter (dc.prog, written by a one-thread
  // kernel per panel) advances -- a slow but live peer (first-call RCCL setup, a long chain-bound fit) is not a dead one (ADVICE r4)
  auto t0 = std::chrono::steady_clock::now();
  int seen = dc.prog ? dc.prog[0] : 0;
  for (long it = 0;; ++it) {
    const hipError_t e = hipEventQuery(dc.ev_wait);
    if (e == hipSuccess) return SIGP_OK;
    if (e != hipErrorNotReady) return fail(h, SIGP_HIP_ERROR, "hipEventQuery failed while waiting for %s: %s", what, hipGetErrorString(e));
    if (dc.prog && dc.prog[0] != seen) { seen = dc.prog[0]; t0 = std::chrono::steady_clock::now(); }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (api && api->CommGetAsyncError && dc.comm && (it & 63) == 63) {
      ncclResult_t ar = ncclSuccess;
      if (api->CommGetAsyncError((ncclComm_t)dc.comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress)
        return dist_mark_dead(h, what, api->GetErrorString ? api->GetErrorString(ar) : "asynchronous RCCL error");
    }
    if (h->opt_dist_timeout_ms > 0 && ms > (double)h->opt_dist_timeout_ms) {
      char why[128];
      snprintf(why, sizeof why, "no progress for %ld ms (dist_timeout_ms): a peer is gone or stalled", (long)h->opt_dist_timeout_ms);
      return dist_mark_dead(h, what, why);
    }
    if (ms > 5.0) std::this_thread::sleep_for(std::chrono::microseconds(100));   // (short fits never get here: they are polled hot)
  }
}

// a transport callback failed / a local error mid-fit: nothing more is enqueued; whatever is in flight is given the deadline to drain
int dist_fail(sigp_handle* h, int rc) {
  auto& dc = h->dc;
  const std::string msg = h->err;
  Slot& s = h->slots[0];
  const auto t0 = std::chrono::steady_clock::now();
  for (hipStream_t st : {s.s_pan, dc.s_comm, s.s_upd}) {
    if (!st) continue;
    while (hipStreamQuery(st) == hipErrorNotReady) {
      if (h->opt_dist_timeout_ms > 0 && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > (double)h->opt_dist_timeout_ms) break;
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
  }
  dc.dead = dc.kind != 0; dc.fit_ok = false; dc.inv_ready = dc.alpha_ready = false;
  h->dl.on = false;
  h->err = msg + " -- the handle's sharded state is dead: sigp_dist_shutdown, then a fresh sigp_dist_init* (the other ranks end in an error of their own within dist_timeout_ms)";
  return rc;
}

// broadcast `bytes` of the device buffer from rank `root`, ordered on `st` (in place)
int dist_bcast(sigp_handle* h, void* dev, size_t bytes, int root, hipStream_t st) {
  auto& dc = h->dc;
  if (dc.kind == 0 || bytes == 0) return SIGP_OK;     // (a one-rank RCCL communicator still runs its collectives: the API path is the same)
  dc.st_collectives += 1;
  if (dc.kind == 1) {
    RcclApi* api = rccl_api(nullptr);
    const auto t0 = std::chrono::steady_clock::now();
    NCCLCHK(h, api, api->Broadcast(dev, dev, bytes, ncclChar, root, (ncclComm_t)dc.comm, st));
    dc.st_host_comm_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SIGP_OK;
  }
  if (dc.tr.device_buffers) {
    if (dc.tr.bcast(dc.tr.ctx, dev, bytes, root, (void*)st)) return fail(h, SIGP_HIP_ERROR, "transport: broadcast callback failed");
    return SIGP_OK;
  }
  int rc = dist_hstage(h, bytes);
  if (rc) return rc;
  if (dc.rank == root) HIPCHK(h, hipMemcpyAsync(dc.hstage, dev, bytes, hipMemcpyDeviceToHost, st));
  if ((rc = dist_wait(h, st, "broadcast (staging)"))) return rc;
  if (dc.tr.bcast(dc.tr.ctx, dc.hstage, bytes, root, nullptr)) return fail(h, SIGP_HIP_ERROR, "transport: broadcast callback failed");
  if (dc.rank != root) {
    HIPCHK(h, hipMemcpyAsync(dev, dc.hstage, bytes, hipMemcpyHostToDevice, st));
    if ((rc = dist_wait(h, st, "broadcast (staging)"))) return rc;      // the staging buffer is reused by the next collective
  }
  return SIGP_OK;
}

// all-reduce `count` elements in place on the device (op 0 = sum, 1 = min), ordered on `st`
int dist_allreduce(sigp_handle* h, void* dev, size_t count, bool f32, int op, hipStream_t st) {
  auto& dc = h->dc;
  if (dc.kind == 0 || count == 0) return SIGP_OK;
  dc.st_collectives += 1;
  if (dc.kind == 1) {
    RcclApi* api = rccl_api(nullptr);
    NCCLCHK(h, api, api->AllReduce(dev, dev, count, f32 ? ncclFloat32 : ncclFloat64, op == 0 ? ncclSum : ncclMin, (ncclComm_t)dc.comm, st));
    return SIGP_OK;
  }
  if (dc.tr.device_buffers) {
    if (dc.tr.allreduce(dc.tr.ctx, dev, count, f32 ? 1 : 0, op, (void*)st)) return fail(h, SIGP_HIP_ERROR, "transport: all-reduce callback failed");
    return SIGP_OK;
  }
  const size_t bytes = count * (f32 ? sizeof(float) : sizeof(double));
  int rc = dist_hstage(h, bytes);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(dc.hstage, dev, bytes, hipMemcpyDeviceToHost, st));
  if ((rc = dist_wait(h, st, "all-reduce (staging)"))) return rc;
  if (dc.tr.allreduce(dc.tr.ctx, dc.hstage, count, f32 ? 1 : 0, op, nullptr)) return fail(h, SIGP_HIP_ERROR, "transport: all-reduce callback failed");
  HIPCHK(h, hipMemcpyAsync(dev, dc.hstage, bytes, hipMemcpyHostToDevice, st));
  if ((rc = dist_wait(h, st, "all-reduce (staging)"))) return rc;
  return SIGP_OK;
}

// scatter from `root`, in place: the root's buffer holds nranks chunks of `chunk` bytes, rank r receives chunk r at dev + r chunk
// (the root keeps its own); ordered on `st`.  RCCL: grouped ncclSend / ncclRecv (one message per directed link).
int dist_scatter(sigp_handle* h, void* dev, size_t chunk, int root, hipStream_t st) {
  auto& dc = h->dc;
  if (dc.kind == 0 || chunk == 0 || dc.nranks < 2) return SIGP_OK;
  dc.st_collectives += 1;
  char* base = (char*)dev;
  if (dc.kind == 1) {
    RcclApi* api = rccl_api(nullptr);
    if (!api->Send || !api->Recv || !api->GroupStart || !api->GroupEnd) return fail(h, SIGP_HIP_ERROR, "librccl lacks ncclSend / ncclRecv / ncclGroup*");
    NCCLCHK(h, api, api->GroupStart());
    // the first error is kept and the group is closed whatever happened: an open group would swallow every later call of this thread,
    // the ncclCommAbort of dist_mark_dead included
    ncclResult_t first = ncclSuccess;
    if (dc.rank == root) {
      for (int r = 0; r < dc.nranks && first == ncclSuccess; ++r)
        if (r != root) first = api->Send(base + (size_t)r * chunk, chunk, ncclChar, r, (ncclComm_t)dc.comm, st);
    } else {
      first = api->Recv(base + (size_t)dc.rank * chunk, chunk, ncclChar, root, (ncclComm_t)dc.comm, st);
    }
    const ncclResult_t ge = api->GroupEnd();
    if (first == ncclSuccess) first = ge;
    if (first != ncclSuccess) return fail(h, SIGP_HIP_ERROR, "RCCL error in the row-piece scatter: %s", api->GetErrorString ? api->GetErrorString(first) : "?");
    return SIGP_OK;
  }
  if (!dc.tr.scatter) return fail(h, SIGP_BAD_ARG, "dist_panel_split: the caller's transport has no scatter callback");
  if (dc.tr.device_buffers) {
    if (dc.tr.scatter(dc.tr.ctx, dev, chunk, root, (void*)st)) return fail(h, SIGP_HIP_ERROR, "transport: scatter callback failed");
    return SIGP_OK;
  }
  int rc = dist_hstage(h, chunk * dc.nranks);
  if (rc) return rc;
  if (dc.rank == root) HIPCHK(h, hipMemcpyAsync(dc.hstage, dev, chunk * dc.nranks, hipMemcpyDeviceToHost, st));
  if ((rc = dist_wait(h, st, "scatter (staging)"))) return rc;
  if (dc.tr.scatter(dc.tr.ctx, dc.hstage, chunk, root, nullptr)) return fail(h, SIGP_HIP_ERROR, "transport: scatter callback failed");
  if (dc.rank != root) {
    HIPCHK(h, hipMemcpyAsync(base + (size_t)dc.rank * chunk, (char*)dc.hstage + (size_t)dc.rank * chunk, chunk, hipMemcpyHostToDevice, st));
    if ((rc = dist_wait(h, st, "scatter (staging)"))) return rc;
  }
  return SIGP_OK;
}

// all-gather in place: rank r contributes chunk r (dev + r chunk), every rank ends with all nranks chunks; ordered on `st`
int dist_allgather(sigp_handle* h, void* dev, size_t chunk, hipStream_t st) {
  auto& dc = h->dc;
  if (dc.kind == 0 || chunk == 0 || dc.nranks < 2) return SIGP_OK;
  dc.st_collectives += 1;
  char* base = (char*)dev;
  if (dc.kind == 1) {
    RcclApi* api = rccl_api(nullptr);
    if (!api->AllGather) return fail(h, SIGP_HIP_ERROR, "librccl lacks ncclAllGather");
    NCCLCHK(h, api, api->AllGather(base + (size_t)dc.rank * chunk, base, chunk, ncclChar, (ncclComm_t)dc.comm, st));
    return SIGP_OK;
  }
  if (!dc.tr.allgather) return fail(h, SIGP_BAD_ARG, "dist_panel_split: the caller's transport has no allgather callback");
  if (dc.tr.device_buffers) {
    if (dc.tr.allgather(dc.tr.ctx, dev, chunk, (void*)st)) return fail(h, SIGP_HIP_ERROR, "transport: all-gather callback failed");
    return SIGP_OK;
  }
  int rc = dist_hstage(h, chunk * dc.nranks);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync((char*)dc.hstage + (size_t)dc.rank * chunk, base + (size_t)dc.rank * chunk, chunk, hipMemcpyDeviceToHost, st));
  if ((rc = dist_wait(h, st, "all-gather (staging)"))) return rc;
  if (dc.tr.allgather(dc.tr.ctx, dc.hstage, chunk, nullptr)) return fail(h, SIGP_HIP_ERROR, "transport: all-gather callback failed");
  for (int r = 0; r < dc.nranks; ++r)
    if (r != dc.rank) HIPCHK(h, hipMemcpyAsync(base + (size_t)r * chunk, (char*)dc.hstage + (size_t)r * chunk, chunk, hipMemcpyHostToDevice, st));
  if ((rc = dist_wait(h, st, "all-gather (staging)"))) return rc;
  return SIGP_OK;
}

// ---- layout ----------------------------------------------------------------------------------------------------------------------
int dl_width(const sigp_handle* h, int q) { return (int)std::min<long>(h->dl.W, h->n_pad / NB - (long)q * h->dl.W); }
template <typename Real>
Real* dl_origin(sigp_handle* h, int q) {      // virtual origin of panel q's columns: element (i, j) = origin[i * ncol + j], j global
  return (Real*)h->dl.mat + h->dl.lcol[(size_t)q] - (long)q * h->dl.W * NB;
}
long dist_panel_elems(const sigp_handle* h, int p) {          // packed panel: the rows BELOW its top block (ride rows included) x its columns --
  return (h->n_pad + RIDE - ((long)p * h->dl.W + dl_width(h, p)) * NB) * (long)dl_width(h, p) * NB;   // nobody else reads the top W x W block
}

template <typename Real>
int shard_begin(sigp_handle* h, int W, int world, int rank) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  const long T = h->n_pad / NB;
  dl.W = W; dl.world = world; dl.rank = rank; dl.P = (int)((T + W - 1) / W);
  dl.lcol.assign((size_t)dl.P, -1);
  long ncol = 0;
  for (int q = 0; q < dl.P; ++q)
    if (q % world == rank) { dl.lcol[(size_t)q] = ncol; ncol += (long)dl_width(h, q) * NB; }
  dl.ncol = std::max<long>(ncol, NB);
  const size_t need = (size_t)(h->n_pad + RIDE) * dl.ncol * sizeof(Real);
  if (dl.cap < need) {
    HIPCHK(h, hipDeviceSynchronize());
    if (dl.mat) HIPCHK(h, hipFree(dl.mat));
    dl.mat = nullptr; dl.cap = 0;
    HIPCHK(h, hipMalloc(&dl.mat, need));
    dl.cap = need;
  }
  const size_t need_d = (size_t)T * NB * NB * sizeof(Real);
  if (dl.cap_dinv < need_d) {
    if (dl.dinv) HIPCHK(h, hipFree(dl.dinv));
    dl.dinv = nullptr; dl.cap_dinv = 0;
    HIPCHK(h, hipMalloc(&dl.dinv, need_d));
    dl.cap_dinv = need_d;
  }
  HIPCHK(h, hipMemsetAsync(dl.dinv, 0, need_d, h->slots[0].s_upd));     // strictly-upper parts stay zero (stream-ordered before everything below)
  // (+ world row blocks: the row-split exchange pads the rows below a panel's top block to `world` equal chunks)
  const size_t need_p = (size_t)(dist_panel_elems(h, 0) + (long)world * NB * dl_width(h, 0) * NB) * sizeof(Real);
  const size_t need_t = (size_t)((long)W * NB * W * NB + (long)W * NB * NB) * sizeof(Real);    // a panel's top block + its inverse diagonal blocks
  if (dc.cap_tbuf < need_t) {
    HIPCHK(h, hipDeviceSynchronize());
    for (int k = 0; k < 2; ++k) { if (dc.tbuf[k]) HIPCHK(h, hipFree(dc.tbuf[k])); dc.tbuf[k] = nullptr; }
    dc.cap_tbuf = 0;
    for (int k = 0; k < 2; ++k) HIPCHK(h, hipMalloc(&dc.tbuf[k], need_t));
    dc.cap_tbuf = need_t;
  }
  if (dc.cap_pbuf < need_p) {
    HIPCHK(h, hipDeviceSynchronize());
    for (int k = 0; k < 2; ++k) {
      if (dc.pbuf[k]) HIPCHK(h, hipFree(dc.pbuf[k]));
      if (dc.sbuf[k]) HIPCHK(h, hipFree(dc.sbuf[k]));
      dc.pbuf[k] = dc.sbuf[k] = nullptr;
    }
    dc.cap_pbuf = 0;
    for (int k = 0; k < 2; ++k) { HIPCHK(h, hipMalloc(&dc.pbuf[k], need_p)); HIPCHK(h, hipMalloc(&dc.sbuf[k], need_p)); }
    dc.cap_pbuf = need_p;
  }
  int rc = dist_streams(h);
  if (rc) return rc;
  Slot& s = h->slots[0];
  if ((rc = slot_reserve(h, s, NB, 1))) return rc;   // res / info / kps buffers
  HIPCHK(h, hipMemsetAsync(s.info, 0, sizeof(int), s.s_upd));
  dl.on = true;
  h->built = h->factored = h->fitted = false;
  return SIGP_OK;
}

// this rank's block columns of K~ and of the ride rows (enqueued on the update stream)
template <typename Real>
int shard_build(sigp_handle* h, int kernel_id, double ell, double sn_tilde, const double* Sigma, int64_t ldsigma) {
  auto& dl = h->dl;
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad, dp = h->dp;
  int rc;
  h->kernel_id = kernel_id; h->sn_tilde = sn_tilde;
  if (kernel_id == SIGP_KERNEL_NETDIFFUSION) {
    if (!std::is_same<Real, double>::value) return fail(h, SIGP_BAD_ARG, "dist_fit: the reference kernel needs the fp64 engine");
    if (!Sigma || ldsigma < h->d) return fail(h, SIGP_BAD_ARG, "dist_fit: Sigma required for the reference kernel");
    h->kp = make_kparams(SIGP_KERNEL_NETDIFFUSION, 1.0, sn_tilde, 0); h->ell = 0;
    if ((rc = sigma_prepare(h, Sigma, ldsigma))) return rc;
    for (int q = 0; q < dl.P; ++q)
      if (dl.lcol[(size_t)q] >= 0 && (rc = sigma_emit(h, (double*)dl_origin<Real>(h, q), dl.ncol, q * dl.W, q * dl.W + dl_width(h, q), sn_tilde))) return rc;
    if ((rc = sigma_kss(h, Sigma, ldsigma))) return rc;
    return SIGP_OK;
  }
  if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "bad kernel_id");
  if (!(ell > 0)) return fail(h, SIGP_BAD_ARG, "ell > 0 required");
  h->kp = make_kparams(kernel_id, ell, sn_tilde, 0); h->ell = ell;
  h->kss_unit.assign((size_t)h->m, 1.0);
  s.kps_host[0] = h->kp;
  if ((rc = upload_kparams(h, s, 1))) return rc;
  bool any = false;
  for (auto c : dl.lcol) any = any || c >= 0;
  if (any) {     // every own block column in ONE launch each for K~ and for the ride rows (local block column x <-> global: the cyclic map)
    const int cyc = dl.W | (dl.world << 8) | (dl.rank << 16);
    const int ncb = (int)(dl.ncol / NB);
    ProfScope ps(h, st, SIGP_KC_KBUILD, (double)n * dl.ncol * (3.0 * h->d + 20) / 2, (double)sizeof(Real) * n * dl.ncol / 2);
    launch_kbuild<Real>(h, dim3((unsigned)ncb, (unsigned)(n_pad / KB_TM), 1), st, h->X, 0L, (int)dp, (int)h->d, (int)n, (Real*)dl.mat, 0L, dl.ncol, s.kps, 16, cyc);
    hipLaunchKernelGGL(ride_build_kernel<Real>, dim3((unsigned)((dl.ncol + 255) / 256), RIDE, 1), dim3(256), 0, st, h->X, 0L, h->Xs, 0L, h->y, 0L, (int)dp,
                       (int)h->d, (int)n, (int)n_pad, (int)h->m, 1, (Real*)dl.mat + n_pad * dl.ncol, 0L, dl.ncol, s.kps, 1, 0, (int)dl.ncol, cyc);
    HIPCHK(h, hipGetLastError());
  }
  return SIGP_OK;
}

// Row-split panel exchange: the rows below a panel's top block, `nrows` 128-row blocks of them at C (row stride ldc = the panel's width),
// against the factored top block L11 [w 128][w 128] (row stride ldc as well) and its inverse diagonal blocks -- X = A21 L11^-T by the
// same binary recursion over the panel's columns, the same tile kernels and the same k order as the owner's whole-panel path
// (panel_rec, sigp_factor.inc), restricted to these rows: bit-identical row for row.
template <typename Real>
int rows_solve(sigp_handle* h, hipStream_t st, Real* Cm, long nrows, long ldc, const Real* L11, const Real* dinvb, int c0, int w) {
  if (nrows <= 0 || w <= 0) return SIGP_OK;
  if (w == 1) {
    GemmArgsT<Real> g{};
    g.A = Cm + (long)c0 * NB; g.lda = ldc;
    g.B = dinvb + (long)c0 * NB * NB; g.ldb = NB;
    g.C = Cm + (long)c0 * NB; g.ldc = ldc;
    return launch_column_solve<Real>(h, st, g, nrows, 1);
  }
  const int hw = w / 2;
  int rc = rows_solve<Real>(h, st, Cm, nrows, ldc, L11, dinvb, c0, hw);
  if (rc) return rc;
  GemmArgsT<Real> g{};
  g.A = Cm + (long)c0 * NB; g.lda = ldc;
  g.B = L11 + (long)(c0 + hw) * NB * ldc + (long)c0 * NB; g.ldb = ldc;
  g.C = Cm + (long)(c0 + hw) * NB; g.ldc = ldc;
  g.batch = 1; g.K = hw * NB; g.r0 = 0; g.r1 = (int)nrows; g.c0 = 0; g.c1 = w - hw; g.lower = 0;
  if ((rc = gemm_sub_auto(h, st, g))) return rc;
  return rows_solve<Real>(h, st, Cm, nrows, ldc, L11, dinvb, c0 + hw, w - hw);
}

// ---- the panel loop -----------------------------------------------------------------------------------------------------------
// Enqueues the whole sharded factorisation; returns without waiting (the caller synchronises once, at the reductions).
template <typename Real>
int shard_factor(sigp_handle* h, bool lookahead) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  Slot& s = h->slots[0];
  const int P = dl.P, me = dl.rank, world = dl.world;
  const long n_pad = h->n_pad;
  const int R = (int)(n_pad / NB) + 1;
  hipStream_t su = s.s_upd;
  hipStream_t sp = lookahead ? s.s_pan : su;       // owner's latency chain
  hipStream_t sc = lookahead ? dc.s_comm : su;     // broadcasts
  const bool stats = h->opt_dist_stats != 0;
  // a host-pointer transport blocks inside dist_bcast: it cannot run ahead of the device anyway
  for (auto e : dc.ev_t) (void)hipEventDestroy(e);
  dc.ev_t.clear();
  auto stamp = [&](hipStream_t st) -> int {
    hipEvent_t e;
    HIPCHK(h, hipEventCreate(&e));
    HIPCHK(h, hipEventRecord(e, st));
    dc.ev_t.push_back(e);
    return SIGP_OK;
  };
  int rc;
  bool read_set[2] = {false, false}, bcast_set[2] = {false, false}, first_set[2] = {false, false}, solve_set[2] = {false, false};
  HIPCHK(h, hipEventRecord(dc.ev_mark, su));       // this rank's columns are built (covariance build, ride rows, dinv memset: all on su)
  // EVERY rank's panel stream starts behind its own build, not only panel 0's owner: the owner of panel 1 applies panel 0's segments
  // to its columns on sp as they arrive (ordered after the collective only), and a rank that entered the fit late -- or whose build
  // is still running when the first segment lands -- would otherwise update columns the build has not written yet
  if (sp != su) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_mark, 0));
  if (stats && (rc = stamp(su))) return rc;        // ev_t[0]: start of the factorisation
  dc.st_bcast_bytes = 0; dc.st_link_bytes = 0; dc.st_split_panels = 0; dc.st_link_panel_max = 0;
  for (auto e : dc.ev_own) (void)hipEventDestroy(e);
  dc.ev_own.clear();
  const int S = std::max(1, h->opt_dist_seg);       // column blocks per broadcast segment
  // which panels take the exchange by row pieces (dist_panel_split; -1 = from four ranks on, where the owner's whole-panel solve is what
  // the other ranks wait for): those with at least two row blocks per rank below their top block, and not the last one
  const bool split_on = h->opt_dist_split > 0 || (h->opt_dist_split < 0 && world >= 4);
  auto split_of = [&](int q) -> bool {
    if (q < 0 || q + 1 >= P || !split_on || dc.kind == 0 || world < 2) return false;
    const long rows_q = n_pad + RIDE - ((long)q * dl.W + dl_width(h, q)) * NB;
    return rows_q / NB >= 2L * world;
  };
  // Row-split panels in a row: the FIRST UPDATE of the next panel's columns is divided by rows as well (dist_lookahead2d).  Panel p + 1 is then
  // scattered with update p still missing below its top block; every rank applies it to its own piece (from the all-gathered panel p) before
  // it solves the piece, and the next owner keeps only what its chain needs: the update of panel p + 1's TOP block, from the `hot` rows of
  // panel p -- the first W row blocks below p's top block, which owner p solves itself right behind its top block and broadcasts on their
  // own -- so that chain p + 1 starts as soon as those arrive, beside the piece solves and the all-gather of panel p.  Per panel the
  // critical path is then  top-block chain + hot rows (update, solve, broadcast) + top-block update  instead of  ... + first update of the
  // whole trapezoid by one rank + piece solves + all-gather.  Same arithmetic per row (a piece's updates arrive in panel order).
  const bool la2d = h->opt_dist_la2d != 0 && sp != su;
  for (int p = 0; p < P; ++p) {
    const int k = p & 1, owner = p % world, Wp = dl_width(h, p), J = p * dl.W;
    // what travels: the rows below the panel's top block (every later panel starts at or below row block J + Wp); the last panel
    // has no reader at all and is neither packed nor broadcast
    const long Jb = (long)J + Wp, rows = n_pad + RIDE - Jb * NB, wcols = (long)Wp * NB;
    const bool travels = p + 1 < P;
    // STREAMED in segments of S column blocks: a segment leaves as soon as its last column is solved, while the owner's chain is
    // still at work on the next columns; the NEXT panel's owner applies each segment to its columns as it arrives (K = S 128),
    // so that when the last segment lands only that one remains between the two owners' chains -- the critical path of a
    // chain-bound sharded fit is then sum(factor) instead of sum(factor + broadcast + first update).  Everyone else assembles the
    // segments into the row-major panel and applies it in one K = W 128 launch as before.  Same k order per tile: bit-identical.
    const long nrb_ = rows / NB;
    const bool split_ = split_of(p);                 // (row-split exchange, below: no segments)
    const int nseg = (travels && !split_) ? (Wp + S - 1) / S : 0;
    Real* buf = (Real*)dc.pbuf[k];                  // row-major [rows][wcols]: operand of the K = W 128 updates of the ranks that received it
    Real* sb = nseg > 1 ? (Real*)dc.sbuf[k] : buf;  // segment g at sb + rows (g S 128): [rows][width_g 128]; one segment = the panel itself
    auto seg_w = [&](int g) { return std::min(S, Wp - g * S); };
    auto seg_ptr = [&](int g) { return sb + rows * ((long)g * S * NB); };
    // Exchange by ROW PIECES (dist_panel_split): the owner factors only the top block; the rows below it -- `nrb` 128-row blocks, the ride
    // block among them -- are cut into `world` equal chunks of `cbk` blocks (the buffer is padded), scattered, solved where they land and
    // all-gathered.  Panels with few rows below, and the last one, keep the whole-panel path.
    const long nrb = nrb_;
    const bool split = split_;
    const long cbk = split ? (nrb + world - 1) / world : 0;
    const size_t chunk_bytes = (size_t)(cbk * NB * wcols) * sizeof(Real);
    const bool from_local = owner == me && !split;  // the owner reads its panel where it was factored: nothing is packed for its own updates
    const bool own_next = p + 1 < P && (p + 1) % world == me;
    const int kprev = (p + 1) & 1;                  // == (p - 1) & 1
    bool comm_stamped = false;
    // the next panel's owner, when it is not this panel's owner: segment g -> its columns, on its panel stream
    auto seg_update = [&](int g) -> int {
      const int q = p + 1, Wq = dl_width(h, q), Jq = q * dl.W;
      const long lda = (long)seg_w(g) * NB, o = (long)Jq * NB;
      GemmArgsT<Real> ga{};
      ga.A = seg_ptr(g) + (o - Jb * NB) * lda; ga.lda = lda;
      ga.B = ga.A; ga.ldb = lda;
      ga.C = dl_origin<Real>(h, q) + o * dl.ncol + o; ga.ldc = dl.ncol;
      ga.batch = 1; ga.K = seg_w(g) * NB; ga.r0 = 0; ga.r1 = R - Jq; ga.c0 = 0; ga.c1 = Wq; ga.lower = 1;
      return gemm_sub_auto(h, sp, ga);
    };
    // (row-distributed first update, see above)  raw_prev: this panel's rows below its top block still lack update p - 1 (iteration p - 1
    // applied it to the top block only); hot: the next panel will be handled the same way, so this panel's first `hot` row blocks below the
    // top block are solved by the owner and broadcast ahead of the pieces
    const bool raw_prev = la2d && split && p > 0 && split_of(p - 1);
    const long hot = (la2d && split && split_of(p + 1)) ? (long)dl_width(h, p + 1) : 0;
    Real* pprev = (Real*)dc.pbuf[kprev];            // panel p - 1 as gathered: rows from p's top block down, row stride = its width
    const long ldprev = p > 0 ? (long)dl_width(h, p - 1) * NB : 0;
    // rows [i0, i0 + nr) (128-row blocks) of this panel's exchange buffer -= (panel p - 1, the same rows) (panel p - 1, the rows of p's top block)^T
    auto piece_update = [&](long i0, long nr) -> int {
      if (nr <= 0) return SIGP_OK;
      GemmArgsT<Real> ga{};
      ga.A = pprev + ((long)Wp + i0) * NB * ldprev; ga.lda = ldprev;
      ga.B = pprev; ga.ldb = ldprev;
      ga.C = buf + i0 * NB * wcols; ga.ldc = wcols;
      ga.batch = 1; ga.K = (int)ldprev; ga.r0 = 0; ga.r1 = (int)nr; ga.c0 = 0; ga.c1 = Wp; ga.lower = 0;
      return gemm_sub_auto(h, sp, ga);
    };
    if (split) {
      Real* tb = (Real*)dc.tbuf[k];
      const size_t top_bytes = (size_t)(wcols * wcols + (long)Wp * NB * NB) * sizeof(Real);
      hipEvent_t own0 = nullptr, own1 = nullptr;
      if (owner == me) {
        // the unsolved rows below the top block -> the exchange buffer (its previous panel's readers first), then out in `world` pieces
        if (bcast_set[k] && sp != sc) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_bcast[k], 0));
        if (read_set[k] && sp != su) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_read[k], 0));
        if (stats) { HIPCHK(h, hipEventCreate(&own0)); HIPCHK(h, hipEventCreate(&own1)); HIPCHK(h, hipEventRecord(own0, sp)); }
        hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, sp,
                           (const char*)((Real*)dl.mat + Jb * NB * dl.ncol + dl.lcol[(size_t)p]), (long)(dl.ncol * sizeof(Real)), (char*)buf, (long)(wcols * sizeof(Real)), rows,
                           (int)(wcols * sizeof(Real)));
        HIPCHK(h, hipGetLastError());
        if (own1) {                                // (two brackets: a blocking host transport idles the panel stream inside the scatter below)
          HIPCHK(h, hipEventRecord(own1, sp)); dc.ev_own.push_back(own0); dc.ev_own.push_back(own1);
          HIPCHK(h, hipEventCreate(&own0)); HIPCHK(h, hipEventCreate(&own1));
        }
        HIPCHK(h, hipEventRecord(dc.ev_pack[k], sp));
        if (sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_pack[k], 0));
      } else {
        if (read_set[k] && sc != su) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_read[k], 0));
        if (first_set[k] && sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_first[k], 0));
        if (solve_set[k] && sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_solve[k], 0));     // (this rank's solve two panels ago read tbuf[k])
        if (solve_set[kprev] && sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_solve[kprev], 0));   // (... and the last panel's piece update read THIS buffer: panel p - 2 as gathered)
      }
      if (stats && (rc = stamp(sc))) return rc;    // ev_t[1 + 4p]
      comm_stamped = true;
      if ((rc = dist_scatter(h, buf, chunk_bytes, owner, sc))) return rc;
      if (owner == me) {
        // ... while the top block is factored (its chain is all that is left on the owner), packed with its inverse diagonal blocks and broadcast
        if (own0) HIPCHK(h, hipEventRecord(own0, sp));
        if ((rc = dist_panel_top<Real>(h, s, dl_origin<Real>(h, p), dl.ncol, (Real*)dl.dinv, sp, J, Wp))) return rc;
        hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((wcols + 3) / 4)), dim3(256), 0, sp,
                           (const char*)((Real*)dl.mat + (long)J * NB * dl.ncol + dl.lcol[(size_t)p]), (long)(dl.ncol * sizeof(Real)), (char*)tb, (long)(wcols * sizeof(Real)), wcols,
                           (int)(wcols * sizeof(Real)));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(tb + wcols * wcols, (const Real*)dl.dinv + (long)J * NB * NB, (size_t)Wp * NB * NB * sizeof(Real), hipMemcpyDeviceToDevice, sp));
        HIPCHK(h, hipEventRecord(dc.ev_pack[k], sp));
        if (sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_pack[k], 0));
        if (hot > 0) {
          // the hot rows, right behind the top block on the owner's chain (from its own packed copy; nothing here waits for a collective of
          // this panel): brought up to date with panel p - 1, solved, and sent out on their own behind the top block
          if (raw_prev) {
            if (sp != sc && bcast_set[kprev]) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_bcast[kprev], 0));   // (panel p - 1 is gathered)
            if ((rc = piece_update(0, hot))) return rc;
          }
          if ((rc = rows_solve<Real>(h, sp, buf, hot, wcols, tb, tb + wcols * wcols, 0, Wp))) return rc;
          HIPCHK(h, hipEventRecord(dc.ev_hot[k], sp));
        }
        if (own1) { HIPCHK(h, hipEventRecord(own1, sp)); dc.ev_own.push_back(own0); dc.ev_own.push_back(own1); }
      }
      if ((rc = dist_bcast(h, tb, top_bytes, owner, sc))) return rc;
      HIPCHK(h, hipEventRecord(dc.ev_seg, sc));
      if (sp != sc) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_seg, 0));
      if (raw_prev && sp != sc && bcast_set[kprev]) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_bcast[kprev], 0));   // panel p - 1 is gathered: the pieces' missing update reads it
      if (hot > 0) {
        if (owner == me && sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_hot[k], 0));
        if ((rc = dist_bcast(h, buf, (size_t)(hot * NB * wcols) * sizeof(Real), owner, sc))) return rc;
        HIPCHK(h, hipEventRecord(dc.ev_hot[k], sc));
        dc.st_bcast_bytes += (owner == me) ? 0.0 : (double)(hot * NB * wcols) * sizeof(Real);
        dc.st_link_bytes += (owner == me) ? (double)(hot * NB * wcols) * sizeof(Real) : 0.0;
      }
      // every rank: its piece of the rows below (without the hot rows), on its panel stream
      const long r0b = (long)me * cbk, nrmine = std::max<long>(0, std::min<long>(cbk, nrb - r0b));
      const long skip = std::min(nrmine, std::max<long>(0, hot - r0b));
      if (raw_prev && (rc = piece_update(r0b + skip, nrmine - skip))) return rc;
      if ((rc = rows_solve<Real>(h, sp, buf + (r0b + skip) * NB * wcols, nrmine - skip, wcols, tb, tb + wcols * wcols, 0, Wp))) return rc;
      HIPCHK(h, hipEventRecord(dc.ev_solve[k], sp));
      solve_set[k] = true;
      if (sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_solve[k], 0));
      if ((rc = dist_allgather(h, buf, chunk_bytes, sc))) return rc;
      dc.st_bcast_bytes += (double)top_bytes * (owner == me ? 0 : 1) + (double)chunk_bytes * (world - 1 + (owner == me ? 0 : 1));   // bytes RECEIVED by this rank
      dc.st_link_bytes += (double)chunk_bytes + (owner == me ? (double)chunk_bytes + (double)top_bytes : 0.0);                       // bytes SENT to one peer
      dc.st_link_panel_max = std::max(dc.st_link_panel_max, (double)chunk_bytes + (owner == me ? (double)chunk_bytes + (double)top_bytes : 0.0));
      dc.st_split_panels += 1;
    } else if (owner == me) {
      // the panel's own columns are up to date: their update with panel p - 1 ran on this panel stream just before (p = 0: the build)
      bool waited = false;
      std::function<int(int)> on_col = [&](int c) -> int {      // column block c of the panel is final (all rows below solved)
        const int i = c - J;
        if (!travels || dc.kind == 0 || !((i + 1) % S == 0 || i == Wp - 1)) return SIGP_OK;
        const int g = i / S, wg = seg_w(g);
        if (!waited) {   // the staging buffer's previous panel (p - 2): its broadcasts and every reader must be done before it is overwritten
          if (bcast_set[k] && sp != sc) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_bcast[k], 0));
          if (read_set[k] && sp != su) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_read[k], 0));
          waited = true;                            // (ev_first[k], this rank's own segment updates, is earlier on sp itself)
        }
        hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, sp,
                           (const char*)((Real*)dl.mat + Jb * NB * dl.ncol + dl.lcol[(size_t)p] + (long)g * S * NB), (long)(dl.ncol * sizeof(Real)), (char*)seg_ptr(g),
                           (long)(wg * NB * sizeof(Real)), rows, (int)(wg * NB * sizeof(Real)));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(dc.ev_pack[k], sp));
        if (sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_pack[k], 0));
        int rcb;
        if (stats && !comm_stamped) { if ((rcb = stamp(sc))) return rcb; comm_stamped = true; }   // ev_t[1 + 4p]: the first segment may leave
        if ((rcb = dist_bcast(h, seg_ptr(g), (size_t)(rows * wg * NB) * sizeof(Real), owner, sc))) return rcb;
        dc.st_bcast_bytes += (double)(rows * wg * NB) * sizeof(Real);
        return SIGP_OK;
      };
      hipEvent_t own0 = nullptr, own1 = nullptr;
      if (stats) { HIPCHK(h, hipEventCreate(&own0)); HIPCHK(h, hipEventCreate(&own1)); HIPCHK(h, hipEventRecord(own0, sp)); }
      if ((rc = dist_panel<Real>(h, s, dl_origin<Real>(h, p), dl.ncol, (Real*)dl.dinv, sp, n_pad, J, Wp, &on_col))) return rc;
      if (own1) { HIPCHK(h, hipEventRecord(own1, sp)); dc.ev_own.push_back(own0); dc.ev_own.push_back(own1); }
      if (travels && dc.kind != 0) {              // (a broadcast puts the whole panel on each of the owner's links)
        dc.st_link_bytes += (double)(rows * wcols) * sizeof(Real);
        dc.st_link_panel_max = std::max(dc.st_link_panel_max, (double)(rows * wcols) * sizeof(Real));
      }
      HIPCHK(h, hipEventRecord(dc.ev_pack[k], sp));   // the panel is factored (the owner's own updates wait for this)
    } else {
      if (read_set[k] && sc != su) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_read[k], 0));
      if (first_set[k] && sc != sp) HIPCHK(h, hipStreamWaitEvent(sc, dc.ev_first[k], 0));   // (segment updates on the panel stream read it as well)
      if (stats && (rc = stamp(sc))) return rc;    // ev_t[1 + 4p]
      comm_stamped = true;
      for (int g = 0; g < nseg; ++g) {
        if ((rc = dist_bcast(h, seg_ptr(g), (size_t)(rows * seg_w(g) * NB) * sizeof(Real), owner, sc))) return rc;
        if (dc.kind != 0) dc.st_bcast_bytes += (double)(rows * seg_w(g) * NB) * sizeof(Real);
        if (own_next && sp != su) {                // this rank factors the next panel: apply the segment to those columns right away
          HIPCHK(h, hipEventRecord(dc.ev_seg, sc));
          if (sp != sc) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_seg, 0));
          if (g == 0 && p > 0 && read_set[kprev]) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_read[kprev], 0));   // the rest of update p - 1 wrote these columns too
          if ((rc = seg_update(g))) return rc;
        }
      }
      if (own_next && sp != su && nseg > 0) { HIPCHK(h, hipEventRecord(dc.ev_first[k], sp)); first_set[k] = true; }
    }
    if (stats && !comm_stamped && (rc = stamp(sc))) return rc;   // (a panel that does not travel)
    HIPCHK(h, hipEventRecord(dc.ev_bcast[k], sc));
    bcast_set[k] = true;
    if (stats && (rc = stamp(sc))) return rc;      // ev_t[2 + 4p]: panel p has arrived / left
    auto update = [&](int q, hipStream_t st) -> int {   // own panel q (> p) -= (panel p)(panel p)^T, all W 128 columns of panel p at once
      const int Wq = dl_width(h, q), Jq = q * dl.W;
      const long lda = from_local ? dl.ncol : wcols, o = (long)Jq * NB;
      GemmArgsT<Real> g{};
      g.A = from_local ? (Real*)dl.mat + o * dl.ncol + dl.lcol[(size_t)p] : buf + (o - Jb * NB) * lda; g.lda = lda;       // rows of panel p from row block Jq down
      g.B = g.A; g.ldb = lda;
      g.C = dl_origin<Real>(h, q) + o * dl.ncol + o; g.ldc = dl.ncol;
      g.batch = 1; g.K = Wp * NB; g.r0 = 0; g.r1 = R - Jq; g.c0 = 0; g.c1 = Wq; g.lower = 1;
      return gemm_sub_auto(h, st, g);
    };
    // the rest of this rank's panels in ONE launch: member z = own panel q0 + z world (all of full width), its trapezoid shifted
    // down by z world W row blocks (GemmArgsT::zshift); rows are counted from panel q0's diagonal block for every member, so
    // A is shared and only the B rows / C columns move with z.  A narrower last panel goes separately.
    auto update_rest = [&](int qfrom) -> int {
      int q0 = -1, cnt = 0, tail = -1;
      for (int q = qfrom; q < P; ++q)
        if (q % world == me) {
          if (dl_width(h, q) < dl.W) { tail = q; continue; }
          if (q0 < 0) q0 = q;
          ++cnt;
        }
      if (cnt > 0) {
        const int Jq = q0 * dl.W;
        const long lda = from_local ? dl.ncol : wcols, o = (long)Jq * NB;
        GemmArgsT<Real> g{};
        g.A = from_local ? (Real*)dl.mat + o * dl.ncol + dl.lcol[(size_t)p] : buf + (o - Jb * NB) * lda; g.lda = lda; g.sA = 0;
        g.B = g.A; g.ldb = lda; g.sB = (long)world * dl.W * NB * lda;
        g.C = (Real*)dl.mat + o * dl.ncol + dl.lcol[(size_t)q0]; g.ldc = dl.ncol; g.sC = (long)dl.W * NB;
        g.batch = cnt; g.K = Wp * NB; g.r0 = 0; g.r1 = R - Jq; g.c0 = 0; g.c1 = dl.W; g.lower = 1; g.zshift = world * dl.W;
        int rcu = gemm_sub_auto(h, su, g);
        if (rcu) return rcu;
      }
      if (tail >= 0) return update(tail, su);
      return SIGP_OK;
    };
    // The next panel's columns first, and on ITS OWNER'S PANEL STREAM: that update, the panel's factorisation and its segments' packs
    // are then one in-order chain (no inter-queue hand-off in it, and the diagonal-block kernel is queued before the rest of the
    // trailing update can occupy every CU); the rest starts on the update stream once this first update is done.  (The
    // first_on_panel schedule of potrf_core, sigp_factor.inc, across ranks.)  When this rank is not panel p's owner the first update was applied segment by
    // segment above; when it is, in one launch from local storage.
    if (own_next && sp != su && split && hot > 0) {
      // row-distributed first update: this rank keeps the update of panel p + 1's TOP block, from the hot rows (the rows below it get theirs
      // piece by piece, wherever they are solved) -- it does not wait for the all-gather
      if (sp != sc) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_hot[k], 0));
      if (p > 0 && read_set[kprev]) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_read[kprev], 0));   // the rest of update p - 1 wrote these columns too
      const int q = p + 1, Wq = dl_width(h, q), Jq = q * dl.W;
      GemmArgsT<Real> g{};
      g.A = buf; g.lda = wcols; g.B = buf; g.ldb = wcols;                                      // (panel p + 1's top block starts at the first row below panel p's)
      g.C = dl_origin<Real>(h, q) + (long)Jq * NB * dl.ncol + (long)Jq * NB; g.ldc = dl.ncol;
      g.batch = 1; g.K = Wp * NB; g.r0 = 0; g.r1 = Wq; g.c0 = 0; g.c1 = Wq; g.lower = 1;
      if ((rc = gemm_sub_auto(h, sp, g))) return rc;
      HIPCHK(h, hipEventRecord(dc.ev_first[k], sp));
      first_set[k] = true;
    } else if (own_next && sp != su && (owner == me || split)) {
      if (split && sp != sc) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_bcast[k], 0));             // (the assembled panel: behind the all-gather)
      if (p > 0 && read_set[kprev]) HIPCHK(h, hipStreamWaitEvent(sp, dc.ev_read[kprev], 0));   // the rest of update p - 1 wrote these columns too
      if ((rc = update(p + 1, sp))) return rc;
      HIPCHK(h, hipEventRecord(dc.ev_first[k], sp));
      first_set[k] = true;
    }
    if (stats && (rc = stamp(su))) return rc;      // ev_t[3 + 4p]: the update stream is ready for panel p
    // the owner updates from its own storage without waiting for the collective to finish
    if (owner == me && !split) { if (su != sp) HIPCHK(h, hipStreamWaitEvent(su, dc.ev_pack[k], 0)); }
    else if (su != sc) HIPCHK(h, hipStreamWaitEvent(su, dc.ev_bcast[k], 0));
    if (split && owner == me) {                    // the assembled rows below the top block -> the owner's storage (later solves read the factor there)
      hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, su, (const char*)buf, (long)(wcols * sizeof(Real)),
                         (char*)((Real*)dl.mat + Jb * NB * dl.ncol + dl.lcol[(size_t)p]), (long)(dl.ncol * sizeof(Real)), rows, (int)(wcols * sizeof(Real)));
      HIPCHK(h, hipGetLastError());
    }
    if (stats && (rc = stamp(su))) return rc;      // ev_t[4 + 4p]: ... and has it
    bool any = false;
    const bool need_rest = p + 2 < P || (own_next && sp == su);
    if (!from_local && nseg > 1 && need_rest) {    // assemble the segments into the row-major panel (one read + one write of it: ~ 0.05 ms)
      for (int g = 0; g < nseg; ++g)
        hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, su, (const char*)seg_ptr(g), (long)(seg_w(g) * NB * sizeof(Real)),
                           (char*)(buf + (long)g * S * NB), (long)(wcols * sizeof(Real)), rows, (int)(seg_w(g) * NB * sizeof(Real)));
      HIPCHK(h, hipGetLastError());
      any = true;
    }
    if (own_next) {
      if (sp != su) { if (first_set[k]) HIPCHK(h, hipStreamWaitEvent(su, dc.ev_first[k], 0)); }
      else if ((rc = update(p + 1, su))) return rc;
      any = true;
    }
    if (p + 2 < P) {
      if ((rc = update_rest(p + 2))) return rc;
      any = true;
    }
    if (any || owner == me) { HIPCHK(h, hipEventRecord(dc.ev_read[k], su)); read_set[k] = true; }     // (the owner's unpack of a row-split panel reads the buffer as well)
    if (dc.prog && dc.kind != 0) {             // (what a timed-out wait reports: the last panel this rank's update stream got through)
      hipLaunchKernelGGL(progress_kernel, dim3(1), dim3(1), 0, su, (volatile int*)dc.prog, p + 1);
      HIPCHK(h, hipGetLastError());
    }
  }
  // join: everything this rank enqueued is behind the update stream
  if (sp != su) { HIPCHK(h, hipEventRecord(s.ev_pan, sp)); HIPCHK(h, hipStreamWaitEvent(su, s.ev_pan, 0)); }
  if (sc != su) { HIPCHK(h, hipEventRecord(s.ev_la, sc)); HIPCHK(h, hipStreamWaitEvent(su, s.ev_la, 0)); }
  if (stats && (rc = stamp(su))) return rc;        // ev_t[1 + 4P]: end of the factorisation
  return SIGP_OK;
}

// after a synchronisation: turn the stamps of shard_factor into the dist_* statistics
void shard_stats(sigp_handle* h) {
  auto& dc = h->dc;
  const int P = h->dl.P;
  dc.st_factor_ms = dc.st_comm_ms = dc.st_stall_ms = dc.st_owner_ms = 0;
  float ms = 0;
  for (size_t i = 0; i + 1 < dc.ev_own.size(); i += 2)
    if (hipEventElapsedTime(&ms, dc.ev_own[i], dc.ev_own[i + 1]) == hipSuccess) dc.st_owner_ms += ms;     // what ONE rank did alone for its panels
  if ((int)dc.ev_t.size() != 2 + 4 * P) return;
  if (hipEventElapsedTime(&ms, dc.ev_t[0], dc.ev_t[(size_t)(1 + 4 * P)]) == hipSuccess) dc.st_factor_ms = ms;
  for (int p = 0; p < P; ++p) {
    if (hipEventElapsedTime(&ms, dc.ev_t[(size_t)(1 + 4 * p)], dc.ev_t[(size_t)(2 + 4 * p)]) == hipSuccess) dc.st_comm_ms += ms;    // broadcast in flight
    if (hipEventElapsedTime(&ms, dc.ev_t[(size_t)(3 + 4 * p)], dc.ev_t[(size_t)(4 + 4 * p)]) == hipSuccess) dc.st_stall_ms += ms;   // update stream idle, waiting for the panel
  }
}

// partial reductions over this rank's columns (epilogue_kernel's layout), summed over the ranks; the pivot info MIN-reduced
template <typename Real>
int shard_reduce(sigp_handle* h, double* res_host, int* info_out) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  HIPCHK(h, hipMemsetAsync(s.res, 0, 512 * sizeof(double), st));
  bool any = false;
  for (auto c : dl.lcol) any = any || c >= 0;
  if (any) {
    const Real* Z = (const Real*)dl.mat + h->n_pad * dl.ncol;
    hipLaunchKernelGGL(epilogue_kernel<Real>, dim3((unsigned)(h->m + 1), 1), dim3(256), 0, st, Z, dl.ncol, Z, (const Real*)nullptr, dl.ncol, (int)h->n,
                       (int)dl.ncol, (int)(h->m + 1), s.res, 0L, 0L, 0L);
    hipLaunchKernelGGL(logdiag_cyclic_kernel<Real>, dim3(1), dim3(256), 0, st, (const Real*)dl.mat, dl.ncol, (int)h->n, (int)dl.ncol,
                       dl.W | (dl.world << 8) | (dl.rank << 16), s.res + 256);
    HIPCHK(h, hipGetLastError());
  }
  hipLaunchKernelGGL(info_to_double_kernel, dim3(1), dim3(1), 0, st, (const int*)s.info, dc.dinfo);
  HIPCHK(h, hipGetLastError());
  int rc;
  if ((rc = dist_allreduce(h, s.res, 512, false, 0, st))) return rc;
  if ((rc = dist_allreduce(h, dc.dinfo, 1, false, 1, st))) return rc;
  // the deadline-polled wait FIRST: a device-to-host copy into pageable memory (di below) blocks inside the runtime until the stream
  // reaches it -- for ever, behind a collective that never completes
  if ((rc = dist_wait(h, st, "fit (panel loop + reductions)"))) return rc;
  double di = 0.0;
  HIPCHK(h, hipMemcpyAsync(s.res_host, s.res, 512 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(&di, dc.dinfo, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  *info_out = di >= 1e17 ? 0 : (int)di;
  memcpy(res_host, s.res_host, 512 * sizeof(double));
  return SIGP_OK;
}

// ---- fp32 engine, sharded: triangular solves with the factor spread over the ranks + fp64 refinement sharded by rows ---------
// Work vectors are PANEL-MAJOR floats [P][TS_RHS][PW], PW = W 128: panel p's piece of every right-hand side is one contiguous
// message.  ft [TS_RHS][ncol] holds this rank's pieces in local-column order (what the column-dot updates in place).
//   backward  x = L^-T t:  for q = P-1 .. 0:  owner: x_q = L_qq^-T t_q (explicit inverse, one skinny product) -> broadcast x_q ->
//             every rank: t[own columns left of q] -= L[rows of q, those columns]^T x_q  (one column-dot over a row block of its storage)
//   forward   z = L^-1 r:  for p = 0 .. P-1:  all-reduce the ranks' accumulated contributions c_p -> owner: z_p = L_pp^-1 (r_p + c_p) ->
//             owner: c[rows below p] -= L[rows below, columns of p] z_p  (one row-dot over its column panel)
// Every step streams a different part of the rank's share of the factor exactly once; the chain per panel is one small
// collective (16 KB) + two skinny kernels.  All of it runs on ONE stream (collectives included): nothing overlaps here, and an
// inter-stream hand-off costs more than the kernels it would order.
template <typename Real>
int shard_solve_reserve(sigp_handle* h) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  const long PW = (long)dl.W * NB;
  int nown = 0;
  for (auto c : dl.lcol) nown += c >= 0;
  const size_t need_inv = (size_t)std::max(nown, 1) * PW * PW * sizeof(Real);
  if (dc.cap_inv < need_inv) {
    for (void** p : {&dc.Uinv, &dc.Vinv}) { if (*p) HIPCHK(h, hipFree(*p)); *p = nullptr; }
    dc.cap_inv = 0;
    HIPCHK(h, hipMalloc(&dc.Uinv, need_inv));
    HIPCHK(h, hipMalloc(&dc.Vinv, need_inv));
    dc.cap_inv = need_inv;
  }
  if (dc.cap_invP < (size_t)PW * PW * sizeof(Real)) {
    if (dc.invP) HIPCHK(h, hipFree(dc.invP));
    dc.invP = nullptr; dc.cap_invP = 0;
    HIPCHK(h, hipMalloc(&dc.invP, (size_t)PW * PW * sizeof(Real)));
    dc.cap_invP = (size_t)PW * PW * sizeof(Real);
  }
  const size_t need_vec = (size_t)dl.P * TS_RHS * PW * sizeof(Real);
  if (dc.cap_vec < need_vec) {
    for (void** p : {&dc.fx, &dc.fr, &dc.fc}) { if (*p) HIPCHK(h, hipFree(*p)); *p = nullptr; }
    dc.cap_vec = 0;
    for (void** p : {&dc.fx, &dc.fr, &dc.fc}) HIPCHK(h, hipMalloc(p, need_vec));
    dc.cap_vec = need_vec;
  }
  const size_t need_ft = (size_t)TS_RHS * dl.ncol * sizeof(Real);
  if (dc.cap_ft < need_ft) {
    if (dc.ft) HIPCHK(h, hipFree(dc.ft));
    dc.ft = nullptr; dc.cap_ft = 0;
    HIPCHK(h, hipMalloc(&dc.ft, need_ft));
    dc.cap_ft = need_ft;
  }
  return SIGP_OK;
}

int shard32_reserve(sigp_handle* h) {
  auto& dc = h->dc;
  int rc = shard_solve_reserve<float>(h);
  if (rc) return rc;
  // the fp64 side: solutions, residuals, partial sums (as the single-GPU fp32 engine's)
  const long n_pad = h->n_pad;
  if (dc.cap_ref_npad < n_pad || !h->xq) {
    for (double** p : {&h->xq, &h->rq, &h->rpart, &h->fpart}) if (*p) { HIPCHK(h, hipFree(*p)); *p = nullptr; }
    dc.cap_ref_npad = 0;
    HIPCHK(h, hipMalloc((void**)&h->xq, (size_t)4 * n_pad * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&h->rq, (size_t)4 * n_pad * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&h->rpart, refine_part_bytes(n_pad)));
    HIPCHK(h, hipMalloc((void**)&h->fpart, (size_t)(n_pad / 256 + 1) * 8 * sizeof(double)));
    dc.cap_ref_npad = n_pad;
  }
  return SIGP_OK;
}

// index of own panel q among this rank's panels
int dl_own_index(const sigp_handle* h, int q) {
  int k = 0;
  for (int i = 0; i < q; ++i) k += h->dl.lcol[(size_t)i] >= 0;
  return k;
}

template <typename Real>
int shard_inverses(sigp_handle* h, hipStream_t st) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  const long PW = (long)dl.W * NB;
  int rc;
  for (int q = 0; q < dl.P; ++q) {
    if (dl.lcol[(size_t)q] < 0) continue;
    const int Wq = dl_width(h, q), J = q * dl.W, k = dl_own_index(h, q);
    const long ldq = (long)Wq * NB;
    Real* U = (Real*)dc.Uinv + (size_t)k * PW * PW;
    Real* V = (Real*)dc.Vinv + (size_t)k * PW * PW;
    int span = 1;
    while (span < Wq) span *= 2;
    const Real* Lq = dl_origin<Real>(h, q) + (long)J * NB * dl.ncol + (long)J * NB;   // the panel's diagonal block in local storage
    if ((rc = trtri_levels<Real>(h, st, Lq, dl.ncol, (const Real*)dl.dinv + (long)J * NB * NB, U, (Real*)dc.invP, ldq, Wq, span))) return rc;
    hipLaunchKernelGGL(transpose_diag_blocks_kernel<Real>, dim3((unsigned)((ldq + 31) / 32), (unsigned)((ldq + 31) / 32), 1), dim3(256), 0, st, (const Real*)U, V, ldq,
                       (int)ldq, (int)ldq);
    HIPCHK(h, hipGetLastError());
  }
  return SIGP_OK;
}

// x (panel-major, replicated on return) = L^-T t; t = dc.ft (this rank's pieces, local-column order; consumed)
template <typename Real>
int shard_backward(sigp_handle* h, hipStream_t st, int nrhs) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  const long PW = (long)dl.W * NB;
  Real* ft = (Real*)dc.ft;
  int rc;
  for (int q = dl.P - 1; q >= 0; --q) {
    const int Wq = dl_width(h, q), J = q * dl.W;
    const int kq = Wq * NB;
    Real* xq = (Real*)dc.fx + (size_t)q * TS_RHS * PW;
    if (dl.lcol[(size_t)q] >= 0) {
      const Real* U = (const Real*)dc.Uinv + (size_t)dl_own_index(h, q) * PW * PW;
      hipLaunchKernelGGL(rowdot_kernel<Real>, dim3((unsigned)((kq + 3) / 4)), dim3(256), 0, st, U, (long)kq, kq, kq, 2, (const Real*)(ft + dl.lcol[(size_t)q]), dl.ncol, xq, PW,
                         nrhs, 0);
      HIPCHK(h, hipGetLastError());
    }
    if ((rc = dist_bcast(h, xq, (size_t)TS_RHS * PW * sizeof(Real), q % dl.world, st))) return rc;
    // own columns left of panel q: a prefix of the local storage
    long nleft = 0;
    for (int i = 0; i < q; ++i) if (dl.lcol[(size_t)i] >= 0) nleft += (long)dl_width(h, i) * NB;
    if (nleft > 0) {
      constexpr int CW = 16 * Vec16<Real>::N;
      hipLaunchKernelGGL(coldot_kernel<Real>, dim3((unsigned)((nleft + CW - 1) / CW)), dim3(256), 0, st, (const Real*)dl.mat + (long)J * NB * dl.ncol, dl.ncol, (int)nleft, kq,
                         (const Real*)xq, PW, ft, dl.ncol, nrhs);
      HIPCHK(h, hipGetLastError());
    }
  }
  return SIGP_OK;
}

// z = L^-1 r; r = dc.fr (panel-major, replicated); z lands in dc.ft (this rank's pieces) -- the input of shard_backward
template <typename Real>
int shard_forward(sigp_handle* h, hipStream_t st, int nrhs) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  const long PW = (long)dl.W * NB, n_pad = h->n_pad;
  Real* ft = (Real*)dc.ft;
  int rc;
  HIPCHK(h, hipMemsetAsync(dc.fc, 0, (size_t)dl.P * TS_RHS * PW * sizeof(Real), st));
  for (int p = 0; p < dl.P; ++p) {
    const int Wp = dl_width(h, p), J = p * dl.W;
    const int kp = Wp * NB;
    Real* cp = (Real*)dc.fc + (size_t)p * TS_RHS * PW;
    if (p > 0 && (rc = dist_allreduce(h, cp, (size_t)TS_RHS * PW, sizeof(Real) == 4, 0, st))) return rc;
    if (dl.lcol[(size_t)p] < 0) continue;
    const Real* V = (const Real*)dc.Vinv + (size_t)dl_own_index(h, p) * PW * PW;
    Real* zp = ft + dl.lcol[(size_t)p];
    hipLaunchKernelGGL(rowdot_kernel<Real>, dim3((unsigned)((kp + 3) / 4)), dim3(256), 0, st, V, (long)kp, kp, kp, 1, (const Real*)((Real*)dc.fr + (size_t)p * TS_RHS * PW), PW, zp,
                       dl.ncol, nrhs, 0, (const Real*)cp);
    const long row0 = (long)J * NB + kp, rem = n_pad - row0;
    if (rem > 0)
      hipLaunchKernelGGL(rowdot_kernel<Real>, dim3((unsigned)((rem + 3) / 4)), dim3(256), 0, st, (const Real*)dl.mat + row0 * dl.ncol + dl.lcol[(size_t)p], dl.ncol, (int)rem, kp, 0,
                         (const Real*)zp, dl.ncol, (Real*)dc.fc, 0L, nrhs, 1, (const Real*)nullptr, (int)PW, (int)row0);
    HIPCHK(h, hipGetLastError());
  }
  return SIGP_OK;
}
int shard32_inverses(sigp_handle* h, hipStream_t st) { return shard_inverses<float>(h, st); }
int shard32_backward(sigp_handle* h, hipStream_t st, int nrhs) { return shard_backward<float>(h, st, nrhs); }
int shard32_forward(sigp_handle* h, hipStream_t st, int nrhs) { return shard_forward<float>(h, st, nrhs); }

// reductions, x0, refinement, results of a sharded fp32 fit (the sharded counterpart of f32_finish)
int shard32_finish(sigp_handle* h, int info, const double* res, double* out, double* mean, double* var) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad, dp = h->dp, d = h->d, m = h->m, ld = n_pad;
  const long PW = (long)dl.W * NB;
  const int nrhs = (int)(1 + m);
  const KParams kp = h->kp;
  const double sn = h->sn_tilde;
  const double inf = std::numeric_limits<double>::infinity();
  if (info != 0) {
    out[0] = inf; out[1] = inf; out[2] = (double)info; out[3] = inf;
    for (long j = 0; j < m; ++j) { if (mean) mean[j] = std::nan(""); if (var) var[j] = std::nan(""); }
    return SIGP_OK;
  }
  int rc;
  if ((rc = shard32_inverses(h, st))) return rc;
  // x0 = L^-T (L^-1 b): the ride rows of the local storage hold this rank's pieces of L^-1 [y k*]
  HIPCHK(h, hipMemsetAsync(dc.ft, 0, (size_t)TS_RHS * dl.ncol * sizeof(float), st));
  HIPCHK(h, hipMemcpy2DAsync(dc.ft, (size_t)dl.ncol * sizeof(float), (const float*)dl.mat + n_pad * dl.ncol, (size_t)dl.ncol * sizeof(float), (size_t)dl.ncol * sizeof(float),
                             (size_t)nrhs, hipMemcpyDeviceToDevice, st));
  if ((rc = shard32_backward(h, st, nrhs))) return rc;
  {
    const long tot = (long)nrhs * n_pad;
    hipLaunchKernelGGL(pm_to_rows_kernel<float>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)dc.fx, h->xq, ld, nrhs, (int)n_pad, (int)PW, 0);
    HIPCHK(h, hipGetLastError());
  }
  // rows [i0, i1) of every residual are this rank's
  const long per = ((n + dl.world - 1) / dl.world + 255) / 256 * 256;
  const int i0 = (int)std::min<long>(n, per * dl.rank), i1 = (int)std::min<long>(n, per * (dl.rank + 1));
  const unsigned nblk = (unsigned)std::max<long>(1, (i1 - i0 + 255) / 256);
  const int want = (int)std::min<long>(REFINE_CHUNKS, std::max<long>(1, 2048 / nblk));
  const int jlen = (int)(((n + want - 1) / want + 63) / 64 * 64);
  const unsigned nchunk = (unsigned)((n + jlen - 1) / jlen);
  std::vector<double> rr((size_t)nrhs * n), yh((size_t)n);
  if ((rc = dist_wait(h, st, "refinement (first solve on the distributed factor)"))) return rc;       // (before a copy into pageable memory: see shard_reduce)
  HIPCHK(h, hipMemcpyAsync(yh.data(), h->y, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  double ymax = -1.0;
  for (int it = 0; it <= h->opt_refine_iters; ++it) {
    HIPCHK(h, hipMemsetAsync(h->rq, 0, (size_t)4 * n_pad * sizeof(double), st));
    if (i1 > i0) {
#define CALL_RES(D) hipLaunchKernelGGL(krefine_residual_kernel<D>, dim3(nblk, nchunk), dim3(256), 0, st, h->X, (int)dp, (int)n, nrhs, (const double*)h->xq, ld, h->rpart, ld, jlen, kp, i0, i1)
      SIGP_DREG_DISPATCH(d, CALL_RES);
#undef CALL_RES
#define CALL_FIN(D) hipLaunchKernelGGL(krefine_finish_kernel<D>, dim3(nblk), dim3(256), 0, st, h->X, h->Xs, h->y, (int)dp, (int)n, nrhs, (const double*)h->rpart, ld, (int)nchunk, h->rq, ld, kp, i0, i1)
      SIGP_DREG_DISPATCH(d, CALL_FIN);
#undef CALL_FIN
      HIPCHK(h, hipGetLastError());
    }
    // every other rank's rows are zero here: the sum IS the gathered residual, exact and in a fixed order
    if ((rc = dist_allreduce(h, h->rq, (size_t)nrhs * n_pad, false, 0, st))) return rc;
    if ((rc = dist_wait(h, st, "refinement (sharded solves + residual all-reduce)"))) return rc;      // (before the copies into pageable memory: see shard_reduce)
    for (int r = 0; r < nrhs; ++r) HIPCHK(h, hipMemcpyAsync(rr.data() + (size_t)r * n, h->rq + (size_t)r * ld, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (ymax < 0) { ymax = 0; for (long i = 0; i < n; ++i) ymax = std::max(ymax, std::fabs(yh[i])); }
    double worst = 0, r0max = 0;
    for (int r = 0; r < nrhs; ++r) {
      double mx = 0; for (long i = 0; i < n; ++i) mx = std::max(mx, std::fabs(rr[(size_t)r * n + i]));
      if (r == 0) r0max = mx;
      worst = std::max(worst, r == 0 ? (ymax > 0 ? mx / ymax : 0.0) : mx);
    }
    h->refine_resid = ymax > 0 ? r0max / ymax : 0.0;
    if (it == h->opt_refine_iters) break;                  // the last pass only measures the residual
    if (h->opt_refine_tol_e > 0 && it > 0 && worst <= std::pow(10.0, -(double)h->opt_refine_tol_e)) break;
    {
      const long tot = (long)TS_RHS * n_pad;
      hipLaunchKernelGGL(pm_from_rows_kernel<float>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const double*)h->rq, ld, (float*)dc.fr, nrhs, (int)n_pad, (int)n, (int)PW);
      HIPCHK(h, hipGetLastError());
    }
    if ((rc = shard32_forward(h, st, nrhs))) return rc;
    if ((rc = shard32_backward(h, st, nrhs))) return rc;
    {
      const long tot = (long)nrhs * n_pad;
      hipLaunchKernelGGL(pm_to_rows_kernel<float>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)dc.fx, h->xq, ld, nrhs, (int)n_pad, (int)PW, 1);
      HIPCHK(h, hipGetLastError());
    }
  }
  // the final fp64 dots: O(n d) on the replicated solutions, the same on every rank
  const unsigned nblk_all = (unsigned)((n + 255) / 256);
#define CALL_DOT(D) hipLaunchKernelGGL(krefine_dots_kernel<D>, dim3(nblk_all), dim3(256), 0, st, h->X, h->Xs, h->y, (int)dp, (int)n, nrhs, (const double*)h->xq, ld, h->fpart, kp)
  SIGP_DREG_DISPATCH(d, CALL_DOT);
#undef CALL_DOT
  HIPCHK(h, hipGetLastError());
  std::vector<double> part((size_t)nblk_all * 8);
  if ((rc = dist_wait(h, st, "refinement (final dots)"))) return rc;
  HIPCHK(h, hipMemcpyAsync(part.data(), h->fpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  double dots0[4] = {0, 0, 0, 0}, dots1[4] = {0, 0, 0, 0};
  for (unsigned b = 0; b < nblk_all; ++b)
    for (int r = 0; r < nrhs; ++r) { dots0[r] += part[(size_t)b * 8 + r]; dots1[r] += part[(size_t)b * 8 + 4 + r]; }
  const double sf = dots0[0] / (double)n;                                   // y^T alpha~ / n
  out[0] = sf;
  out[1] = 0.5 * n + res[256] + 0.5 * n * std::log(sf) + 0.5 * n * std::log(2.0 * M_PI);   // log-det from the fp32 factor (summed over the ranks)
  out[2] = 0.0; out[3] = sf * sn;
  for (long j = 0; j < m; ++j) {
    if (mean) mean[j] = dots0[1 + j];                                       // k*^T alpha~
    if (var) var[j] = sf * (1.0 + sn - dots1[1 + j]);                       // k** + sn~ - k*^T K~^-1 k*
  }
  return SIGP_OK;
}

// the whole sharded fit
template <typename Real>
int shard_fit(sigp_handle* h, int kernel_id, double ell, double sn_tilde, const double* Sigma, int64_t ldsigma, int W, bool lookahead, double* out,
              double* mean, double* var) {
  auto& dc = h->dc;
  Slot& s = h->slots[0];
  int rc;
  if (dc.dead) return fail(h, SIGP_HIP_ERROR, "dist_fit: this handle's communicator died in an earlier call (sigp_dist_shutdown, then a fresh sigp_dist_init*)");
  // Argument checks FIRST, before anything is enqueued or any collective is entered: a bad hyper-parameter (an optimiser proposing
  // l <= 0, say) is SIGP_BAD_ARG on every rank alike and leaves the handle usable -- only failures after this point can strand peers
  // inside collectives and take the dist_fail exit (ADVICE r4).
  if (kernel_id == SIGP_KERNEL_NETDIFFUSION) {
    if (!std::is_same<Real, double>::value) return fail(h, SIGP_BAD_ARG, "dist_fit: the reference kernel needs the fp64 engine");
    if (!Sigma || ldsigma < h->d) return fail(h, SIGP_BAD_ARG, "dist_fit: Sigma required for the reference kernel");
  } else {
    if (kernel_id != SIGP_KERNEL_RBF && kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "bad kernel_id");
    if (!(ell > 0) || !std::isfinite(ell)) return fail(h, SIGP_BAD_ARG, "ell > 0 required");
  }
  if (!(sn_tilde >= 0) || !std::isfinite(sn_tilde)) return fail(h, SIGP_BAD_ARG, "sn_tilde >= 0 required");
  if ((h->opt_dist_split > 0 || (h->opt_dist_split < 0 && dc.nranks >= 4)) && dc.kind == 2 && (!dc.tr.scatter || !dc.tr.allgather))
    return fail(h, SIGP_BAD_ARG, "dist_fit: dist_panel_split = 1 needs a transport with scatter and allgather callbacks");
  if (std::is_same<Real, float>::value) {
    if (h->m > 3) return fail(h, SIGP_BAD_ARG, "fp32 engine: at most 3 ride-along test points (refinement solves 1+m systems)");
    if (h->d > 64) return fail(h, SIGP_BAD_ARG, "fp32 engine: d <= 64 required");
  }
  if ((rc = shard_begin<Real>(h, W, dc.nranks, dc.rank))) return rc;
  if (dc.prog) dc.prog[0] = 0;
  if (std::is_same<Real, float>::value && (rc = shard32_reserve(h))) return rc;
  dc.st_collectives = 0; dc.st_host_comm_ms = 0;
  dc.fit_ok = dc.inv_ready = dc.alpha_ready = false;
  const auto t0 = std::chrono::steady_clock::now();
  // a failure from here on (a transport callback, a HIP error, a collective that never completes) leaves the other ranks inside
  // collectives this rank will not join: they end in an error of their own within dist_timeout_ms; this handle is marked dead
  if ((rc = shard_build<Real>(h, kernel_id, ell, sn_tilde, Sigma, ldsigma))) return dist_fail(h, rc);
  if ((rc = shard_factor<Real>(h, lookahead))) return dist_fail(h, rc);
  dc.st_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  double res[512];
  int info = 0;
  if ((rc = shard_reduce<Real>(h, res, &info))) return dc.dead ? rc : dist_fail(h, rc);
  const auto t1 = std::chrono::steady_clock::now();
  if (std::is_same<Real, float>::value) {
    if ((rc = shard32_finish(h, info, res, out, mean, var))) return dc.dead ? rc : dist_fail(h, rc);
  } else {
    finish_results(res, info, h->n, h->m, h->sn_tilde, h->kss_unit.data(), out, mean, var);
  }
  const auto t2 = std::chrono::steady_clock::now();
  dc.st_fit_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
  dc.st_solve_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
  if (h->opt_dist_stats) shard_stats(h);
  h->sigma_f = out[0]; h->nlml = out[1];
  h->built = h->factored = h->fitted = false;      // the factor is spread over the ranks: sigp_predict / sigp_get_alpha do not apply (sigp_dist_predict does)
  dc.fit_ok = info == 0;
  dc.inv_ready = info == 0 && std::is_same<Real, float>::value;   // (the fp32 refinement formed the own diagonal blocks' inverses)
  (void)s;
  if (info != 0) return fail(h, SIGP_NOT_SPD, "dist_fit: matrix is not positive definite (pivot %d)", info);
  return SIGP_OK;
}

// Predictions at NEW points after a sharded fit (north/June1st.py:272-277 for one large K~ whose factor is spread over the ranks):
//   mean_j = k~*_j^T alpha~            alpha~ = K~^-1 y replicated once per fit (fp64: one backward solve on the distributed factor
//                                      from the solved ride row; fp32: the refined solution the fit already holds)
//   var_j  = sigma_f (1 + sn~ - |L~^-1 k~*_j|^2)   up to TS_RHS points per forward solve on the distributed factor; every rank sums the
//                                      squares of its own columns, ONE all-reduce over all m points at the end
// Collective: every rank calls it with the same Xs.  RBF / Matern.
template <typename Real>
int shard_predict(sigp_handle* h, const double* Xs, int64_t m, int64_t ldxs, double* mean, double* var) {
  auto& dl = h->dl;
  auto& dc = h->dc;
  Slot& s = h->slots[0];
  hipStream_t st = s.s_upd;
  const long n = h->n, n_pad = h->n_pad, dp = h->dp, d = h->d, PW = (long)dl.W * NB;
  int rc;
  if ((rc = shard_solve_reserve<Real>(h))) return rc;
  if (!dc.inv_ready) {
    if ((rc = shard_inverses<Real>(h, st))) return rc;
    dc.inv_ready = true;
  }
  if (dc.cap_alpha < (size_t)std::max<long>(n_pad, 1)) {     // (a handle re-used with a larger training set: the buffer follows n_pad)
    if (dc.alpha) HIPCHK(h, hipFree(dc.alpha));
    dc.alpha = nullptr; dc.cap_alpha = 0;
    HIPCHK(h, hipMalloc((void**)&dc.alpha, (size_t)std::max<long>(n_pad, 1) * sizeof(double)));
    dc.cap_alpha = (size_t)std::max<long>(n_pad, 1);
  }
  if (!dc.alpha_ready) {
    if (std::is_same<Real, float>::value) {
      HIPCHK(h, hipMemcpyAsync(dc.alpha, h->xq, (size_t)n_pad * sizeof(double), hipMemcpyDeviceToDevice, st));     // row 0 of the refined solutions
    } else {
      HIPCHK(h, hipMemsetAsync(dc.ft, 0, (size_t)TS_RHS * dl.ncol * sizeof(Real), st));
      HIPCHK(h, hipMemcpyAsync(dc.ft, (const Real*)dl.mat + n_pad * dl.ncol, (size_t)dl.ncol * sizeof(Real), hipMemcpyDeviceToDevice, st));   // z = L~^-1 y, own pieces
      if ((rc = shard_backward<Real>(h, st, 1))) return rc;
      hipLaunchKernelGGL(pm_to_rows_kernel<Real>, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, st, (const Real*)dc.fx, dc.alpha, n_pad, 1, (int)n_pad, (int)PW, 0);
      HIPCHK(h, hipGetLastError());
    }
    dc.alpha_ready = true;
  }
  if (dc.cap_pred < (size_t)(2 * m)) {
    if (dc.pred) HIPCHK(h, hipFree(dc.pred));
    dc.pred = nullptr; dc.cap_pred = 0;
    HIPCHK(h, hipMalloc((void**)&dc.pred, (size_t)(2 * m) * sizeof(double)));
    dc.cap_pred = (size_t)(2 * m);
  }
  HIPCHK(h, hipMemsetAsync(dc.pred, 0, (size_t)(2 * m) * sizeof(double), st));
  const long xs_off = TS_RHS * std::max<long>(ldxs, dp);
  if ((rc = ensure(h, &h->stage, &h->cap_stage, xs_off + TS_RHS * dp))) return rc;
  double* xs_dev = h->stage + xs_off;
  bool any = false;
  for (auto c : dl.lcol) any = any || c >= 0;
  for (long c0 = 0; c0 < m; c0 += TS_RHS) {
    const int mc = (int)std::min<long>(TS_RHS, m - c0);
    HIPCHK(h, hipMemcpyAsync(h->stage, Xs + c0 * ldxs, (size_t)((mc - 1) * ldxs + d) * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)((TS_RHS * dp + 255) / 256)), dim3(256), 0, st, h->stage, (long)ldxs, mc, (int)d, xs_dev, TS_RHS, (int)dp);
    hipLaunchKernelGGL(cross_mean_kernel, dim3((unsigned)mc), dim3(256), 0, st, h->X, xs_dev, (int)dp, (int)d, (int)n, (const double*)dc.alpha, dc.pred + c0, h->kp);
    hipLaunchKernelGGL(cross_cov_pm_kernel<Real>, dim3((unsigned)((TS_RHS * n_pad + 255) / 256)), dim3(256), 0, st, h->X, xs_dev, (int)dp, (int)d, (int)n, (int)n_pad, mc,
                       (Real*)dc.fr, (int)PW, h->kp);
    HIPCHK(h, hipGetLastError());
    if ((rc = shard_forward<Real>(h, st, mc))) return rc;
    if (any) {
      hipLaunchKernelGGL(rowsq_kernel<Real>, dim3((unsigned)mc), dim3(256), 0, st, (const Real*)dc.ft, dl.ncol, (int)dl.ncol, dc.pred + m + c0);
      HIPCHK(h, hipGetLastError());
    }
    if ((rc = dist_wait(h, st, "predict (forward solve on the distributed factor)"))) return rc;          // the staging buffer is refilled by the next chunk
  }
  if ((rc = dist_allreduce(h, dc.pred + m, (size_t)m, false, 0, st))) return rc;
  std::vector<double> res((size_t)(2 * m));
  if ((rc = dist_wait(h, st, "predict (variance all-reduce)"))) return rc;
  HIPCHK(h, hipMemcpyAsync(res.data(), dc.pred, (size_t)(2 * m) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  for (long j = 0; j < m; ++j) {
    mean[j] = res[(size_t)j];
    var[j] = h->sigma_f * (1.0 + h->sn_tilde - res[(size_t)(m + j)]);
  }
  return SIGP_OK;
}
