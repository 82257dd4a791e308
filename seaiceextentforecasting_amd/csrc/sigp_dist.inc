// C ABI of the sharded fit (included by sigp.hip inside extern "C"); the engine is sigp_shard.inc.

int64_t sigp_num_blocks(sigp_handle* h) { return h ? h->n_pad / NB : 0; }

int sigp_dist_unique_id(void* id128) {
  if (!id128) return SIGP_BAD_ARG;
  std::string why;
  RcclApi* api = rccl_api(&why);
  if (!api) return SIGP_HIP_ERROR;
  ncclUniqueId id;
  if (api->GetUniqueId(&id) != ncclSuccess) return SIGP_HIP_ERROR;
  memcpy(id128, &id, sizeof id);
  return SIGP_OK;
}

int sigp_dist_init(sigp_handle* h, int nranks, int rank, const void* nccl_id) {
  if (!h || nranks < 1 || nranks > 255 || rank < 0 || rank >= nranks || (nranks > 1 && !nccl_id)) return fail(h, SIGP_BAD_ARG, "dist_init: bad argument (1 <= nranks <= 255)");
  HIPCHK(h, hipSetDevice(h->device));
  auto& dc = h->dc;
  if (dc.comm) {
    RcclApi* api0 = rccl_api(nullptr);
    if (api0) (void)api0->CommDestroy((ncclComm_t)dc.comm);
    dc.comm = nullptr;
  }
  dc.kind = 0; dc.nranks = nranks; dc.rank = rank;
  // the communication stream BEFORE the communicator: RCCL creates streams of its own, and a stream created once the process has
  // used up its hardware queues (GPU_MAX_HW_QUEUES) shares one with an earlier stream -- a broadcast waiting for a panel would
  // then hold back the update stream's kernels queued behind it (measured: 42 instead of 31 ms at n = 16384)
  {
    int rc0 = dist_streams(h);
    if (rc0) return rc0;
  }
  if (nccl_id) {        // (nranks == 1 with an id: a one-rank communicator -- every collective of the fit still goes through RCCL)
    std::string why;
    RcclApi* api = rccl_api(&why);
    if (!api) return fail(h, SIGP_HIP_ERROR, "dist_init: %s", why.c_str());
    ncclUniqueId id;
    memcpy(&id, nccl_id, sizeof id);
    ncclComm_t comm = nullptr;
    NCCLCHK(h, api, api->CommInitRank(&comm, nranks, id, rank));     // (on failure kind stays 0: sigp_dist_fit then refuses to run with nranks > 1)
    dc.comm = (void*)comm;
    dc.kind = 1;
  }
  return dist_streams(h);
}

int sigp_dist_init_transport2(sigp_handle* h, int nranks, int rank, const sigp_transport* tr, int64_t struct_bytes);
int sigp_dist_init_transport(sigp_handle* h, int nranks, int rank, const sigp_transport* tr) {
  return sigp_dist_init_transport2(h, nranks, rank, tr, (int64_t)sizeof(sigp_transport));
}
// the same with the size of the CALLER's struct: members the caller's header did not have yet (a 3.x caller: scatter / allgather) read as NULL
// instead of whatever follows the shorter struct in memory
int sigp_dist_init_transport2(sigp_handle* h, int nranks, int rank, const sigp_transport* tr, int64_t struct_bytes) {
  sigp_transport t{};
  if (tr) {
    if (struct_bytes < (int64_t)(offsetof(sigp_transport, allreduce) + sizeof(t.allreduce))) return fail(h, SIGP_BAD_ARG, "dist_init_transport: the transport struct is shorter than its first four members");
    memcpy(&t, tr, (size_t)std::min<int64_t>(struct_bytes, (int64_t)sizeof t));
    tr = &t;
  }
  if (!h || nranks < 1 || nranks > 255 || rank < 0 || rank >= nranks || (nranks > 1 && (!tr || !tr->bcast || !tr->allreduce))) return fail(h, SIGP_BAD_ARG, "dist_init_transport: bad argument (1 <= nranks <= 255)");
  HIPCHK(h, hipSetDevice(h->device));
  auto& dc = h->dc;
  if (dc.comm) {
    RcclApi* api0 = rccl_api(nullptr);
    if (api0) (void)api0->CommDestroy((ncclComm_t)dc.comm);
    dc.comm = nullptr;
  }
  dc.nranks = nranks; dc.rank = rank;
  dc.kind = nranks > 1 ? 2 : 0;
  if (tr) dc.tr = *tr;
  return dist_streams(h);
}

int sigp_dist_shutdown(sigp_handle* h) {
  if (!h) return SIGP_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  dist_release(h);
  return SIGP_OK;
}

int sigp_dist_fit(sigp_handle* h, int kernel_id, double ell, double sn_tilde, const double* Sigma, int64_t ldsigma, int64_t W, int lookahead,
                  double* out, double* mean, double* var) {
  if (!h || h->n == 0 || !out) return fail(h, SIGP_BAD_ARG, "dist_fit: call set_train first");
  if (h->ard_on) return fail(h, SIGP_BAD_ARG, "dist_fit: per-feature length scales are set (single-GPU fits only)");
  if (h->opt_accurate) return fail(h, SIGP_BAD_ARG, "dist_fit: option accurate_solve is set (single-GPU fp64 fits only)");
  if (W < 1 || W > 64) return fail(h, SIGP_BAD_ARG, "dist_fit: panel width must be 1..64 blocks");
  if (!(sn_tilde >= 0)) return fail(h, SIGP_BAD_ARG, "sn_tilde >= 0 required");
  if (h->m > 0 && (!mean || !var)) return fail(h, SIGP_BAD_ARG, "dist_fit: mean / var buffers required for the ride-along test points");
  if (h->dc.nranks > 1 && h->dc.kind == 0) return fail(h, SIGP_BAD_ARG, "dist_fit: %d ranks but no transport (sigp_dist_init / sigp_dist_init_transport failed or was not called)", h->dc.nranks);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->dtype == SIGP_F64) return shard_fit<double>(h, kernel_id, ell, sn_tilde, Sigma, ldsigma, (int)W, lookahead != 0, out, mean, var);
  return shard_fit<float>(h, kernel_id, ell, sn_tilde, Sigma, ldsigma, (int)W, lookahead != 0, out, mean, var);
}

int sigp_dist_predict(sigp_handle* h, const double* Xs, int64_t m, int64_t ldxs, double* mean, double* var) {
  if (!h || !Xs || m < 1 || !mean || !var || ldxs < h->d) return fail(h, SIGP_BAD_ARG, "dist_predict: bad argument");
  if (h->ard_on) return fail(h, SIGP_BAD_ARG, "dist_predict: per-feature length scales are set (single-GPU fits only)");
  if (h->dc.dead) return fail(h, SIGP_HIP_ERROR, "dist_predict: this handle's communicator died in an earlier call (sigp_dist_shutdown, then a fresh sigp_dist_init*)");
  if (!h->dl.on || !h->dc.fit_ok) return fail(h, SIGP_BAD_ARG, "dist_predict: no successful sigp_dist_fit on this handle");
  if (h->kernel_id != SIGP_KERNEL_RBF && h->kernel_id != SIGP_KERNEL_MATERN52) return fail(h, SIGP_BAD_ARG, "dist_predict: RBF / MATERN52 fits only (the reference kernel's test points ride along the fit)");
  HIPCHK(h, hipSetDevice(h->device));
  const int rc = h->dtype == SIGP_F64 ? shard_predict<double>(h, Xs, m, ldxs, mean, var) : shard_predict<float>(h, Xs, m, ldxs, mean, var);
  return (rc != SIGP_OK && !h->dc.dead) ? dist_fail(h, rc) : rc;
}
