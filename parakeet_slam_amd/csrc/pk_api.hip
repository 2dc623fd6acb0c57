// C ABI of the FastSLAM particle update (include/parakeet_slam.h) on top of the gfx950
// kernels.  Host orchestration only: argument checks, host<->device staging, launch
// order, hipEvent instrumentation.  No arithmetic of the path runs on the host except
// the three reductions to scalars that the reference also does in Python floats
// (summary's division and atan2, prkt_core_v2.py:273-275) and the per-blob unit ray
// direction cos/sin (prkt_core_v2.py:510), which are O(B), not O(P*L).
// This file: the filter's lifecycle and transfers, motion, resample, the step, the new-landmark bookkeeping, options, timing and
// the probe.  The observe pipeline is pk_api_observe.hip, the multi-GPU protocol pk_api_shard.hip, the path estimate pk_api_path.hip,
// adaptive resampling pk_api_adaptive.hip, the odometry motion model pk_api_odom.hip; pk_filter.hpp is what they share.
#include "pk_filter.hpp"

extern "C" {
int pk_download_landmarks(pk_filter* f, int64_t p0, int64_t p1, double* means, double* covs, int32_t* counts);
int pk_upload_landmarks(pk_filter* f, int64_t p0, int64_t p1, const double* means, const double* covs, const int32_t* counts);
}

#ifdef PK_STAMPS
namespace pk { void debug_read_stamps(unsigned long long* out, bool reset); void debug_read_fused_stamps(unsigned long long* out, bool reset); void debug_read_regs_stamps(unsigned long long* out, bool reset); void debug_read_pub_stamps(unsigned long long* out, bool reset); void debug_read_pub_wave_stamps(unsigned long long* out, bool reset); }
#endif

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int materialise(pk_filter* f) {
  if (f->src_identity) return PK_OK;
  {
    Span t(f, PK_T_MATERIALISE);
    launch_materialise(f->stream, f->d);
  }
  f->src_identity = true;
  f->d.alt = nullptr;  // every slot now lives in the shard's own buffer
  return PK_OK;
}

namespace {

int drain_timings(pk_filter* f) {
  if (f->pending.empty()) return PK_OK;
  PK_HIP(hipStreamSynchronize(f->stream));
  for (auto& t : f->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
      f->ms[t.slot] += ms;
      f->launches[t.slot] += 1;
    }
    f->pool.push_back(t.a);
    f->pool.push_back(t.b);
  }
  f->pending.clear();
  return PK_OK;
}

// Pack one landmark (dense 5x5 host form) into the compact fields of a host slot image.
void pack_landmark(const MapLayout& lay, unsigned char* slot, int l, const double* mean, const double* cov) {
  double* fl = reinterpret_cast<double*>(slot);
  const int Lp = lay.Lp;
  for (int i = 0; i < 5; ++i) fl[(size_t)i * Lp + l] = mean[i];
  if (lay.fields == kDenseFields) {  // the reference's full state, entry by entry
    for (int i = 0; i < 25; ++i) fl[(size_t)(5 + i) * Lp + l] = cov[i];
    return;
  }
  fl[(size_t)F_PXX * Lp + l] = cov[0];
  fl[(size_t)F_PXY * Lp + l] = 0.5 * (cov[1] + cov[5]);
  fl[(size_t)F_PYY * Lp + l] = cov[6];
  fl[(size_t)F_CRR * Lp + l] = cov[12];
  fl[(size_t)F_CRG * Lp + l] = 0.5 * (cov[13] + cov[17]);
  fl[(size_t)F_CRB * Lp + l] = 0.5 * (cov[14] + cov[22]);
  fl[(size_t)F_CGG * Lp + l] = cov[18];
  fl[(size_t)F_CGB * Lp + l] = 0.5 * (cov[19] + cov[23]);
  fl[(size_t)F_CBB * Lp + l] = cov[24];
}

void unpack_landmark(const MapLayout& lay, const unsigned char* slot, int l, double* mean, double* cov) {
  const double* fl = reinterpret_cast<const double*>(slot);
  const int Lp = lay.Lp;
  if (mean)
    for (int i = 0; i < 5; ++i) mean[i] = fl[(size_t)i * Lp + l];
  if (cov && lay.fields == kDenseFields) {
    for (int i = 0; i < 25; ++i) cov[i] = fl[(size_t)(5 + i) * Lp + l];
  } else if (cov) {
    for (int i = 0; i < 25; ++i) cov[i] = 0.0;
    cov[0] = fl[(size_t)F_PXX * Lp + l];
    cov[1] = cov[5] = fl[(size_t)F_PXY * Lp + l];
    cov[6] = fl[(size_t)F_PYY * Lp + l];
    cov[12] = fl[(size_t)F_CRR * Lp + l];
    cov[13] = cov[17] = fl[(size_t)F_CRG * Lp + l];
    cov[14] = cov[22] = fl[(size_t)F_CRB * Lp + l];
    cov[18] = fl[(size_t)F_CGG * Lp + l];
    cov[19] = cov[23] = fl[(size_t)F_CGB * Lp + l];
    cov[24] = fl[(size_t)F_CBB * Lp + l];
  }
}

// 0: fits the compact layout (block diagonal xy (+) rgb, symmetric); 1: finite but needs the dense layout
// (xy-rgb coupling, or not symmetric); PK_ERR_INVALID: not finite.
int classify_covariance(const double* cov, int l) {
  double scale = 0.0;
  for (int i = 0; i < 25; ++i) {
    if (!std::isfinite(cov[i])) return fail(PK_ERR_INVALID, "landmark %d: covariance not finite", l + 1);
    if (i % 6 == 0) scale = fmax(scale, fabs(cov[i]));
  }
  const double tol = 1e-9 * (scale > 0 ? scale : 1.0);
  for (int i = 0; i < 2; ++i)
    for (int j = 2; j < 5; ++j)
      if (fabs(cov[i * 5 + j]) > 1e-14 * scale || fabs(cov[j * 5 + i]) > 1e-14 * scale) return 1;
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j)
      if (fabs(cov[i * 5 + j] - cov[j * 5 + i]) > tol) return 1;
  return 0;
}

// The compact layout stores Sigma = Pxy (+) C: reject anything else loudly.
int check_block_diagonal(const double* cov, int l) {
  double scale = 0.0;
  for (int i = 0; i < 5; ++i) scale = fmax(scale, fabs(cov[i * 6]));
  if (!(scale >= 0.0) || !std::isfinite(scale))
    return fail(PK_ERR_INVALID, "landmark %d: covariance diagonal is not finite", l + 1);
  const double tol = 1e-9 * (scale > 0 ? scale : 1.0);
  for (int i = 0; i < 2; ++i)
    for (int j = 2; j < 5; ++j)
      if (fabs(cov[i * 5 + j]) > 1e-14 * scale || fabs(cov[j * 5 + i]) > 1e-14 * scale)
        return fail(PK_ERR_UNSUPPORTED,
                    "landmark %d: covariance couples position and colour (entry [%d][%d]); the compact "
                    "device layout holds xy 2x2 (+) rgb 3x3 only",
                    l + 1, i, j);
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j) {
      if (!std::isfinite(cov[i * 5 + j])) return fail(PK_ERR_INVALID, "landmark %d: covariance not finite", l + 1);
      if (fabs(cov[i * 5 + j] - cov[j * 5 + i]) > tol)
        return fail(PK_ERR_UNSUPPORTED, "landmark %d: covariance is not symmetric", l + 1);
    }
  return PK_OK;
}

// Switch the filter's maps between the compact (14-row) and the dense (30-row) layout.  keep: the particles' landmark
// states survive (through the host, in chunks: a rare, slow path -- a coupled Qt set after the map, coupled covariances
// uploaded into a compact filter); otherwise the maps are simply reallocated (pk_upload_map refills them).
int relayout(pk_filter* f, bool dense, bool keep) {
  if (f->dense == dense) return PK_OK;
  int rc;
  DeviceState& d = f->d;
  const MapLayout old = d.lay;
  const MapLayout neu = MapLayout::make(old.L, sizeof(double), dense ? kDenseFields : (int)F_COUNT_FIELDS);
  const int64_t P = d.P;
  const int L = old.L;
  std::vector<double> means, covs;
  std::vector<int32_t> counts;
  if (keep && L > 0) {
    if ((rc = materialise(f))) return rc;
    if (!dense)  // dense -> compact drops what the compact layout cannot hold: only when nothing is coupled
      return fail(PK_ERR_STATE, "relayout: a dense map cannot be folded back into the compact layout");
    try {  // the conversion goes through the host (a rare path): P L 30 doubles -- 48 GB at 100 000 x 2 000
      means.resize((size_t)P * L * 5);
      covs.resize((size_t)P * L * 25);
      counts.resize((size_t)P * L);
    } catch (const std::bad_alloc&) {
      return fail(PK_ERR_NOMEM, "relayout: no host memory to stage %lld x %d landmarks for the layout conversion", (long long)P, L);
    }
    if ((rc = pk_download_landmarks(f, 0, P, means.data(), covs.data(), counts.data()))) return rc;
  }
  if ((rc = ct_end(f))) return rc;  // (the buffers go: nothing left to write rows into)
  PK_HIP(hipStreamSynchronize(f->stream));
  for (int i = 0; i < 2; ++i) dev_free(f, &d.map[i]);
  dev_free(f, &f->slot_tmp);
  d.lay = neu;
  f->dense = dense;
  d.alt = nullptr;
  for (int i = 0; i < 2; ++i) {
    if ((rc = dev_alloc(f, &d.map[i], (size_t)P * neu.slot_bytes))) return rc;
    PK_HIP(hipMemsetAsync(d.map[i], 0, (size_t)P * neu.slot_bytes, f->stream));
  }
  if ((rc = dev_alloc(f, &f->slot_tmp, neu.slot_bytes))) return rc;
  launch_iota(f->stream, d.src[0], P);
  launch_iota(f->stream, d.src[1], P);
  f->src_identity = true;
  d.mcur = 0;
  if (keep && L > 0) {
    const bool was_loaded = f->map_loaded;
    f->map_loaded = true;
    rc = pk_upload_landmarks(f, 0, P, means.data(), covs.data(), counts.data());
    f->map_loaded = was_loaded;
    if (rc) return rc;
  }
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

}  // namespace

extern "C" {

int pk_abi_version(void) { return PK_ABI_VERSION; }

const char* pk_status_string(int status) {
  switch (status) {
    case PK_OK: return "ok";
    case PK_ERR_INVALID: return "invalid argument";
    case PK_ERR_HIP: return "HIP runtime error";
    case PK_ERR_STATE: return "invalid call order";
    case PK_ERR_UNSUPPORTED: return "unsupported by the device path";
    case PK_ERR_NOMEM: return "out of memory";
    default: return "unknown status";
  }
}

const char* pk_last_error(void) { return g_last_error.c_str(); }

int pk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int pk_create(int64_t P, int32_t L, int32_t device, pk_filter** out) {
  if (!out) return fail(PK_ERR_INVALID, "pk_create: out is NULL");
  *out = nullptr;
  if (P < 1 || P > 2147483647LL) return fail(PK_ERR_INVALID, "pk_create: num_particles %lld out of range", (long long)P);
  if (L < 0 || L > (1 << 24)) return fail(PK_ERR_INVALID, "pk_create: num_landmarks %d out of range", L);
  int ndev = pk_device_count();
  if (ndev <= 0) return fail(PK_ERR_HIP, "pk_create: no HIP device visible (the HIP path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(PK_ERR_INVALID, "pk_create: device %d of %d", device, ndev);
  pk_filter* f = new (std::nothrow) pk_filter;
  if (!f) return fail(PK_ERR_NOMEM, "pk_create: host allocation failed");
  f->device = device;
  int rc = PK_OK;
  auto bail = [&](int code) {
    pk_destroy(f);
    return code;
  };
  if ((rc = use_device(f))) return bail(rc);
  if (hipStreamCreateWithFlags(&f->own_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(PK_ERR_HIP, "hipStreamCreate failed"));
  f->stream = f->own_stream;
  DeviceState& d = f->d;
  d.P = P;
  d.lay = MapLayout::make(L, sizeof(double));
  d.cur = 0;
  d.mcur = 0;
  f->nblocks = (P + kScanBlock - 1) / kScanBlock;
  for (int i = 0; i < 2 && !rc; ++i) {
    if (!rc) rc = dev_alloc(f, &d.x[i], (size_t)P);
    if (!rc) rc = dev_alloc(f, &d.y[i], (size_t)P);
    if (!rc) rc = dev_alloc(f, &d.h[i], (size_t)P);
    if (!rc) rc = dev_alloc(f, &d.logw[i], (size_t)P);
    if (!rc) rc = dev_alloc(f, &d.src[i], (size_t)P);
    if (!rc) rc = dev_alloc(f, &d.map[i], (size_t)P * d.lay.slot_bytes);
  }
  if (!rc) rc = dev_alloc(f, &d.immutable, (size_t)d.lay.Lp);
  if (!rc) rc = dev_alloc(f, &f->z_dev, (size_t)P * 3);
  if (!rc) rc = dev_alloc(f, &f->partial, (size_t)4 * 1024);
  if (!rc) rc = dev_alloc(f, &f->gmax, 1);
  if (!rc) rc = dev_alloc(f, &f->clocal, (size_t)P);
  if (!rc) rc = dev_alloc(f, &f->totals, (size_t)f->nblocks);
  if (!rc) rc = dev_alloc(f, &f->offsets, (size_t)f->nblocks);
  if (!rc) rc = dev_alloc(f, &f->sum, 1);
  if (!rc) rc = dev_alloc(f, &f->out4, 4);
  if (!rc) rc = dev_alloc(f, &f->pose_part, (size_t)(4 * motion_pose_blocks(P)));
  if (!rc) rc = dev_alloc(f, &f->anc, (size_t)P);
  if (!rc) rc = dev_alloc(f, &f->slot_tmp, d.lay.slot_bytes);
  if (rc) return bail(rc);
  hipError_t e = hipSuccess;
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    e = hipMemsetAsync(d.x[i], 0, P * sizeof(double), f->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d.y[i], 0, P * sizeof(double), f->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d.h[i], 0, P * sizeof(double), f->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d.logw[i], 0, P * sizeof(double), f->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d.map[i], 0, (size_t)P * d.lay.slot_bytes, f->stream);
  }
  if (e == hipSuccess) e = hipMemsetAsync(d.immutable, 0, d.lay.Lp, f->stream);
  if (e != hipSuccess) return bail(fail(PK_ERR_HIP, "pk_create: memset failed: %s", hipGetErrorString(e)));
  launch_iota(f->stream, d.src[0], P);
  launch_iota(f->stream, d.src[1], P);
  if (hipStreamSynchronize(f->stream) != hipSuccess) return bail(fail(PK_ERR_HIP, "pk_create: sync failed"));
  f->map_loaded = (L == 0);
  *out = f;
  return PK_OK;
}

int pk_destroy(pk_filter* f) {
  if (!f) return PK_OK;
  (void)hipSetDevice(f->device);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  for (auto& t : f->pending) {
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  for (auto e : f->pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : f->stage_done)
    if (e) (void)hipEventDestroy(e);
  f->mem.release_all();
  if (f->own_stream) (void)hipStreamDestroy(f->own_stream);
  delete f;
  return PK_OK;
}

int pk_set_stream(pk_filter* f, void* hip_stream) {
  if (!f) return fail(PK_ERR_INVALID, "pk_set_stream: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = drain_timings(f))) return rc;
  PK_HIP(hipStreamSynchronize(f->stream));
  f->stream = hip_stream ? (hipStream_t)hip_stream : f->own_stream;
  return PK_OK;
}

int pk_synchronize(pk_filter* f) {
  if (!f) return fail(PK_ERR_INVALID, "pk_synchronize: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipStreamSynchronize(f->stream));
  return unique_error(f, "pk_synchronize");
}

int64_t pk_num_particles(const pk_filter* f) { return f ? f->d.P : -1; }
int32_t pk_num_landmarks(const pk_filter* f) { return f ? f->d.lay.L : -1; }
int64_t pk_device_bytes(const pk_filter* f) { return f ? (int64_t)f->mem.device_bytes() : -1; }

int pk_set_measurement_noise(pk_filter* f, const double Qt[16]) {
  if (!f || !Qt) return fail(PK_ERR_INVALID, "pk_set_measurement_noise: NULL argument");
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(Qt[i])) return fail(PK_ERR_INVALID, "Qt is not finite");
  double scale = 0;
  for (int i = 0; i < 4; ++i) scale = fmax(scale, fabs(Qt[i * 5]));
  // Qt = [q00] (+) symmetric 3x3 is what the compact layout and the fast kernels take; anything else (bearing-colour
  // coupling, asymmetry -- the reference accepts any 4x4, prkt_core_v2.py:50-53, :817-818) needs the dense kernels
  bool coupled = false;
  for (int j = 1; j < 4; ++j)
    if (fabs(Qt[j]) > 1e-14 * scale || fabs(Qt[j * 4]) > 1e-14 * scale) coupled = true;
  for (int i = 1; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (fabs(Qt[i * 4 + j] - Qt[j * 4 + i]) > 1e-9 * (scale > 0 ? scale : 1.0)) coupled = true;
  int rc;
  if ((rc = use_device(f))) return rc;
  // (the table's levels were made under the old Qt: once an update has used them the mode ends; before that -- scans that matched
  // nothing included: every count is 0 still -- the mode stays and ct_engage builds the table afresh)
  if (f->ct_updated) {
    bool untouched = false;
    if (f->ct_eligible && f->ct_built && !coupled && (rc = ct_maps_untouched(f, &untouched))) return rc;
    if (untouched) f->ct_updated = false;
    else if ((rc = ct_end(f))) return rc;
  }
  if (coupled && !f->dense && (rc = relayout(f, true, f->map_loaded))) return rc;
  for (int i = 0; i < 16; ++i) f->qt16[i] = Qt[i];
  f->qt_dense = coupled;
  f->qt = NoiseD{Qt[0], Qt[5], 0.5 * (Qt[6] + Qt[9]), 0.5 * (Qt[7] + Qt[13]), Qt[10], 0.5 * (Qt[11] + Qt[14]), Qt[15]};
  return PK_OK;
}

int pk_upload_map(pk_filter* f, const double* means, const double* covs, const uint8_t* immutable) {
  if (!f) return fail(PK_ERR_INVALID, "pk_upload_map: NULL handle");
  const MapLayout& lay = f->d.lay;
  const int L = lay.L;
  if (L > 0 && (!means || !covs)) return fail(PK_ERR_INVALID, "pk_upload_map: NULL means/covs");
  int rc;
  if ((rc = use_device(f))) return rc;
  bool need_dense = f->qt_dense;
  for (int l = 0; l < L; ++l) {
    for (int i = 0; i < 5; ++i)
      if (!std::isfinite(means[l * 5 + i])) return fail(PK_ERR_INVALID, "landmark %d: mean is not finite", l + 1);
    const int c = classify_covariance(covs + (size_t)l * 25, l);
    if (c < 0) return c;
    need_dense |= c == 1;  // xy-rgb coupling or asymmetry: the whole filter takes the dense layout and kernels
  }
  if ((rc = relayout(f, need_dense, false))) return rc;  // (lay refers to f->d.lay: the new layout from here on)
  std::vector<unsigned char> slot(lay.slot_bytes, 0);
  std::vector<unsigned char> imm((size_t)lay.Lp, 0);
  for (int l = 0; l < L; ++l) {
    pack_landmark(lay, slot.data(), l, means + (size_t)l * 5, covs + (size_t)l * 25);
    imm[l] = immutable ? (immutable[l] != 0) : 0;
  }
  PK_HIP(hipMemcpyAsync(f->slot_tmp, slot.data(), lay.slot_bytes, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipMemcpyAsync(f->d.immutable, imm.data(), imm.size(), hipMemcpyHostToDevice, f->stream));
  launch_broadcast_slot(f->stream, f->d, f->slot_tmp);
  // every particle holds this map with update counts 0: the colour table's level 0 (the 512-lane publish / subscribe route only)
  f->colour_rows_valid = true;  // (every slot of the live buffer was just rewritten)
  f->ct_engaged = false;
  f->ct_built = false;
  f->ct_updated = false;
  f->ct_eligible = false;
  if (!f->dense && lay.Lp > 2 * kPubSmallThreads && L <= kRegsMaxL) {
    if ((rc = dev_lazy(f, &f->ct_base, (size_t)6 * lay.Lp))) return rc;
    PK_HIP(hipMemcpyAsync(f->ct_base, slot.data() + (size_t)F_CRR * lay.Lp * sizeof(double), (size_t)6 * lay.Lp * sizeof(double),
                          hipMemcpyHostToDevice, f->stream));
    f->ct_eligible = true;
  }
  PK_HIP(hipStreamSynchronize(f->stream));  // host staging buffers die here
  f->src_identity = true;
  f->map_loaded = true;
  return PK_OK;
}

int pk_upload_poses(pk_filter* f, const double* xyhw) {
  poses_change(f);
  if (!f || !xyhw) return fail(PK_ERR_INVALID, "pk_upload_poses: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  const int64_t P = f->d.P;
  std::vector<double> soa((size_t)P * 4);
  for (int64_t i = 0; i < P; ++i) {
    soa[i] = xyhw[4 * i];
    soa[P + i] = xyhw[4 * i + 1];
    soa[2 * P + i] = xyhw[4 * i + 2];
    double w = xyhw[4 * i + 3];
    if (!(w >= 0.0) || !std::isfinite(w)) return fail(PK_ERR_INVALID, "pk_upload_poses: weight of particle %lld is negative, infinite or NaN", (long long)i);
    soa[3 * P + i] = std::log(w);
  }
  const int c = f->d.cur;
  PK_HIP(hipMemcpyAsync(f->d.x[c], soa.data(), P * 8, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipMemcpyAsync(f->d.y[c], soa.data() + P, P * 8, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipMemcpyAsync(f->d.h[c], soa.data() + 2 * P, P * 8, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipMemcpyAsync(f->d.logw[c], soa.data() + 3 * P, P * 8, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  f->gmax_fused = false;
  path_clear(f);  // a replaced population has no lineage
  return PK_OK;
}

/* One particle's pose and weight (FastSLAM.particles[i] = p, prkt_core_v2.py:162): the other particles' log-weights are not
 * touched -- a round trip of ALL poses through their linear weights (pk_download_poses / pk_upload_poses) loses every weight that
 * underflows as exp(log w). */
int pk_upload_pose(pk_filter* f, int64_t p, const double xyhw[4]) {
  if (!f || !xyhw) return fail(PK_ERR_INVALID, "pk_upload_pose: NULL argument");
  if (p < 0 || p >= f->d.P) return fail(PK_ERR_INVALID, "pk_upload_pose: particle %lld of %lld", (long long)p, (long long)f->d.P);
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(xyhw[i])) return fail(PK_ERR_INVALID, "pk_upload_pose: pose component %d is not finite", i);
  // (+inf passed "w >= 0", and log(inf) turns the log-domain scan into NaN / all-zero weights)
  if (!(xyhw[3] >= 0.0) || !std::isfinite(xyhw[3])) return fail(PK_ERR_INVALID, "pk_upload_pose: the weight is negative, infinite or NaN");
  int rc;
  if ((rc = use_device(f))) return rc;
  f->pose_part_ok = false;
  const double v4[4] = {xyhw[0], xyhw[1], xyhw[2], std::log(xyhw[3])};
  const int c = f->d.cur;
  double* const dst[4] = {f->d.x[c] + p, f->d.y[c] + p, f->d.h[c] + p, f->d.logw[c] + p};
  for (int i = 0; i < 4; ++i) PK_HIP(hipMemcpyAsync(dst[i], &v4[i], 8, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  f->gmax_fused = false;
  return PK_OK;
}

int pk_download_poses(pk_filter* f, double* xyhw) {
  if (!f || !xyhw) return fail(PK_ERR_INVALID, "pk_download_poses: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  const int64_t P = f->d.P;
  std::vector<double> soa((size_t)P * 4);
  const int c = f->d.cur;
  PK_HIP(hipMemcpyAsync(soa.data(), f->d.x[c], P * 8, hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipMemcpyAsync(soa.data() + P, f->d.y[c], P * 8, hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipMemcpyAsync(soa.data() + 2 * P, f->d.h[c], P * 8, hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipMemcpyAsync(soa.data() + 3 * P, f->d.logw[c], P * 8, hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  for (int64_t i = 0; i < P; ++i) {
    xyhw[4 * i] = soa[i];
    xyhw[4 * i + 1] = soa[P + i];
    xyhw[4 * i + 2] = soa[2 * P + i];
    xyhw[4 * i + 3] = std::exp(soa[3 * P + i]);
  }
  return PK_OK;
}

int pk_download_log_weights(pk_filter* f, double* logw) {
  if (!f || !logw) return fail(PK_ERR_INVALID, "pk_download_log_weights: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(logw, f->d.logw[f->d.cur], (size_t)f->d.P * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

/* The log-weights of every particle, bit for bit (pk_upload_poses takes log(w): exp and log do not round-trip): what a snapshot
 * of a filter whose weights carry over between resamples restores.  -inf is a weight of zero; NaN and +inf are refused. */
int pk_upload_log_weights(pk_filter* f, const double* logw) {
  if (!f || !logw) return fail(PK_ERR_INVALID, "pk_upload_log_weights: NULL argument");
  for (int64_t i = 0; i < f->d.P; ++i)
    if (!(logw[i] < INFINITY)) return fail(PK_ERR_INVALID, "pk_upload_log_weights: the log-weight of particle %lld is +inf or NaN", (long long)i);
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(f->d.logw[f->d.cur], logw, (size_t)f->d.P * sizeof(double), hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  f->gmax_fused = false;
  return PK_OK;
}

int pk_download_landmarks(pk_filter* f, int64_t p0, int64_t p1, double* means, double* covs, int32_t* counts) {
  if (!f) return fail(PK_ERR_INVALID, "pk_download_landmarks: NULL handle");
  if (p0 < 0 || p1 < p0 || p1 > f->d.P) return fail(PK_ERR_INVALID, "pk_download_landmarks: bad particle range");
  if (!f->map_loaded) return fail(PK_ERR_STATE, "pk_download_landmarks: no map uploaded");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = materialise(f))) return rc;
  if ((rc = colour_rows_for_download(f, p0, p1))) return rc;  // (the colour table's mode goes on)
  const MapLayout& lay = f->d.lay;
  const int L = lay.L;
  const int64_t chunk = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)lay.slot_bytes);
  std::vector<unsigned char> host((size_t)std::min<int64_t>(chunk, p1 - p0) * lay.slot_bytes);
  for (int64_t q0 = p0; q0 < p1; q0 += chunk) {
    int64_t q1 = std::min(p1, q0 + chunk);
    PK_HIP(hipMemcpyAsync(host.data(), f->d.map[f->d.mcur] + (size_t)q0 * lay.slot_bytes,
                          (size_t)(q1 - q0) * lay.slot_bytes, hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    for (int64_t q = q0; q < q1; ++q) {
      const unsigned char* slot = host.data() + (size_t)(q - q0) * lay.slot_bytes;
      const int32_t* cnt = reinterpret_cast<const int32_t*>(slot + lay.count_off);
      for (int l = 0; l < L; ++l) {
        size_t o = (size_t)(q - p0) * L + l;
        unpack_landmark(lay, slot, l, means ? means + o * 5 : nullptr, covs ? covs + o * 25 : nullptr);
        if (counts) counts[o] = cnt[l];
      }
    }
  }
  return PK_OK;
}

int pk_upload_landmarks(pk_filter* f, int64_t p0, int64_t p1, const double* means, const double* covs,
                        const int32_t* counts) {
  if (!f) return fail(PK_ERR_INVALID, "pk_upload_landmarks: NULL handle");
  if (p0 < 0 || p1 < p0 || p1 > f->d.P) return fail(PK_ERR_INVALID, "pk_upload_landmarks: bad particle range");
  if (!f->map_loaded) return fail(PK_ERR_STATE, "pk_upload_landmarks: no map uploaded");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ct_end(f))) return rc;  // (a particle's map edited by hand: its colour blocks are no longer the table's)
  if ((rc = materialise(f))) return rc;
  const int L = f->d.lay.L;
  // finite means and covariances whatever the layout (as pk_upload_map checks them); the layout decision only while compact
  if (means)
    for (int64_t o = 0; o < (p1 - p0) * L * 5; ++o)
      if (!std::isfinite(means[o])) return fail(PK_ERR_INVALID, "pk_upload_landmarks: mean of landmark %d not finite", (int)((o / 5) % L) + 1);
  if (covs) {
    bool need_dense = false;
    for (int64_t o = 0; o < (p1 - p0) * L; ++o) {
      const int c = classify_covariance(covs + (size_t)o * 25, (int)(o % L));
      if (c < 0) return c;
      need_dense |= c == 1;
    }
    if (need_dense && !f->dense && (rc = relayout(f, true, true))) return rc;
  }
  const MapLayout& lay = f->d.lay;  // (after the conversion)
  const int64_t chunk = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)lay.slot_bytes);
  std::vector<unsigned char> host;
  try {
    host.resize((size_t)std::min<int64_t>(chunk, p1 - p0) * lay.slot_bytes);
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "pk_upload_landmarks: no host memory for the staging buffer");
  }
  for (int64_t q0 = p0; q0 < p1; q0 += chunk) {
    int64_t q1 = std::min(p1, q0 + chunk);
    unsigned char* dev = f->d.map[f->d.mcur] + (size_t)q0 * lay.slot_bytes;
    PK_HIP(hipMemcpyAsync(host.data(), dev, (size_t)(q1 - q0) * lay.slot_bytes, hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    for (int64_t q = q0; q < q1; ++q) {
      unsigned char* slot = host.data() + (size_t)(q - q0) * lay.slot_bytes;
      int32_t* cnt = reinterpret_cast<int32_t*>(slot + lay.count_off);
      for (int l = 0; l < L; ++l) {
        size_t o = (size_t)(q - p0) * L + l;
        double m[5], c[25];
        unpack_landmark(lay, slot, l, m, c);
        pack_landmark(lay, slot, l, means ? means + o * 5 : m, covs ? covs + o * 25 : c);
        if (counts) cnt[l] = counts[o];
      }
    }
    PK_HIP(hipMemcpyAsync(dev, host.data(), (size_t)(q1 - q0) * lay.slot_bytes, hipMemcpyHostToDevice, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
  }
  return PK_OK;
}

int pk_reset_weights(pk_filter* f) {
  if (!f) return fail(PK_ERR_INVALID, "pk_reset_weights: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  launch_reset_weights(f->stream, f->d);
  f->gmax_fused = false;
  PK_LAUNCH_CHECK("pk_reset_weights");
  return PK_OK;
}

int pk_motion(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed, uint64_t draw) {
  if (!f) return fail(PK_ERR_INVALID, "pk_motion: NULL handle");
  if (!std::isfinite(v) || !std::isfinite(w) || !std::isfinite(dt)) return fail(PK_ERR_INVALID, "pk_motion: non-finite control");
  return motion_impl(f, "pk_motion", z, [&](const double* zd, void* up_dst, const void* up_src, size_t up_bytes) {
    launch_motion(f->stream, f->d, v, w, dt, zd, seed, draw, 0, up_dst, up_src, up_bytes, f->pose_part);
  });
}

int pk_motion_range(pk_filter* f, double v, double w, double dt, uint64_t seed, uint64_t draw, int64_t p0, int64_t p1) {
  poses_change(f);
  if (!f) return fail(PK_ERR_INVALID, "pk_motion_range: NULL handle");
  if (!std::isfinite(v) || !std::isfinite(w) || !std::isfinite(dt)) return fail(PK_ERR_INVALID, "pk_motion_range: non-finite control");
  if (p0 < 0 || p1 < p0 || p1 > f->d.P) return fail(PK_ERR_INVALID, "pk_motion_range: bad particle range [%lld, %lld)", (long long)p0, (long long)p1);
  int rc;
  if ((rc = use_device(f))) return rc;
  Span t(f, PK_T_MOTION);
  launch_motion_range(f->stream, f->d, v, w, dt, seed, draw, p0, p1);
  PK_LAUNCH_CHECK("pk_motion_range");
  return PK_OK;
}

// The knobs are rows of kOptionTable (pk_filter.hpp, beside their defaults); what follows the loop is not tuning: an option with a
// side effect, protocol state of the sharded tests whose bounds depend on P, and one process-wide setting.
int pk_set_option(pk_filter* f, const char* name, int64_t value) {
  if (!f || !name) return fail(PK_ERR_INVALID, "pk_set_option: NULL argument");
  for (const OptionRow& o : kOptionTable) {
    if (strcmp(name, o.name)) continue;
    if (o.take == Take::Range && (value < o.lo || value > o.hi)) return fail(PK_ERR_INVALID, "%s", o.refusal);
    f->opt.*o.member = o.take == Take::Range ? (int)value : (o.take == Take::Tri && value < 0) ? -1 : (value != 0 ? 1 : 0);
    return PK_OK;
  }
  if (!strcmp(name, "colour_table")) {
    if (value < -1 || value > 1) return fail(PK_ERR_INVALID, "colour_table: -1 (auto), 0 (off) or 1 (as auto)");
    f->opt.colour_table = (int)value;
    if (value == 0 && !f->colour_rows_valid) {  // (switched off in mid-run: the slots get their rows back)
      int rc;
      if ((rc = use_device(f)) || (rc = ct_end(f))) return rc;
    }
    return PK_OK;
  }
  if (!strcmp(name, "split_loopback_lo") || !strcmp(name, "split_loopback_hi")) {
    // debug (one-rank tests of the exchange): the next split adoption fills only the LOCAL slots [lo, hi) of this shard with its
    // own particles directly; the slots outside are filled from records -- which the caller packs with pk_shard_pack_slots_dev
    // and sends through the all-to-all to itself.  Cleared by pk_shard_adopt_remote_dev.
    if (value < 0 || value > f->d.P) return fail(PK_ERR_INVALID, "%s: 0..P", name);
    (name[15] == 'l' ? f->loop_lo : f->loop_hi) = value;
    return PK_OK;
  }
  if (!strcmp(name, "balanced_loopback_keep")) {
    if (value < -1 || value > f->d.P) return fail(PK_ERR_INVALID, "balanced_loopback_keep: -1 (off) .. P");
    f->bal_loop_keep = value;
    return PK_OK;
  }
  if (!strcmp(name, "observe_landmarks_per_lane")) {
    if (value < 0 || value > 2) return fail(PK_ERR_INVALID, "observe_landmarks_per_lane: 0 (default), 1 or 2");
    g_observe_nv = (int)value;
    return PK_OK;
  }
  return fail(PK_ERR_INVALID, "pk_set_option: unknown option '%s'", name);
}

int pk_resample(pk_filter* f, double u, int32_t weight_domain, int64_t* ancestors_out) {
  poses_change(f);
  if (!f) return fail(PK_ERR_INVALID, "pk_resample: NULL handle");
  if (!(u >= 0.0 && u < 1.0)) return fail(PK_ERR_INVALID, "pk_resample: u = %g outside [0,1)", u);
  if (weight_domain != PK_WEIGHTS_LINEAR && weight_domain != PK_WEIGHTS_LOG)
    return fail(PK_ERR_INVALID, "pk_resample: weight_domain %d", weight_domain);
  if (f->split.active) return fail(PK_ERR_STATE, "pk_resample: a split observe is in progress (half the particles observed)");
  if (int refused = refuse_balanced(f, "pk_resample")) return refused;
  int rc;
  if ((rc = use_device(f))) return rc;
  DeviceState& d = f->d;
  {
    Span t(f, PK_T_WEIGHTS);
    const unsigned long long* key = nullptr;
    if (weight_domain == PK_WEIGHTS_LOG) {
      if (f->gmax_fused)
        key = ctl_gmax_key(f);  // the observe kernels kept the max of the weights they wrote
      else
        launch_block_max(f->stream, d, f->partial, f->gmax);
    }
    launch_scan_local(f->stream, d, f->gmax, weight_domain, f->clocal, f->totals, key);
    if (f->nblocks <= kAncestorsScanMaxBlocks) {  // k_ancestors scans the few block totals itself: one launch less
      launch_ancestors(f->stream, f->clocal, f->totals, nullptr, nullptr, f->nblocks, d.P, d.P, u, 0, d.P, f->anc, &d);
    } else {
      launch_scan_blocks(f->stream, f->totals, f->nblocks, f->offsets, f->sum);
      launch_ancestors(f->stream, f->clocal, f->totals, f->offsets, f->sum, f->nblocks, d.P, d.P, u, 0, d.P, f->anc, &d);
    }
  }
  if (f->retire.on()) launch_retire_gather(f->stream, f->grow, f->retire, f->anc, d.P);  // (pk_grow_retire: the clocks too)
  if (f->grow_on) launch_grow_gather(f->stream, f->grow, f->anc, d.P);  // the bookkeeping follows the particles (:243)
  if (f->path.cap && (rc = path_record(f))) return rc;  // the generation that was resampled and its ancestors, into the ring
  PK_LAUNCH_CHECK("pk_resample");
  f->src_identity = false;
  f->gmax_fused = false;
  if (ancestors_out) {
    std::vector<int32_t> a((size_t)d.P);
    PK_HIP(hipMemcpyAsync(a.data(), f->anc, (size_t)d.P * 4, hipMemcpyDeviceToHost, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    for (int64_t i = 0; i < d.P; ++i) ancestors_out[i] = a[i];
  }
  return PK_OK;
}

int pk_summary(pk_filter* f, double out[3]) {
  if (!f || !out) return fail(PK_ERR_INVALID, "pk_summary: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  {
    Span t(f, PK_T_SUMMARY);
    launch_summary_partials(f->stream, f->d, f->partial, f->out4);
  }
  double s[4];
  PK_HIP(hipMemcpyAsync(s, f->out4, sizeof(s), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  const double n = (double)f->d.P;  // prkt_core_v2.py:262
  out[0] = s[0] / n;                // :273
  out[1] = s[1] / n;                // :274
  out[2] = std::atan2(s[2], s[3]);  // :275
  return PK_OK;
}

int pk_pose_sums(pk_filter* f, double out[4]) {
  if (!f || !out) return fail(PK_ERR_INVALID, "pk_pose_sums: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  {
    Span t(f, PK_T_SUMMARY);
    launch_summary_partials(f->stream, f->d, f->partial, f->out4);
  }
  PK_HIP(hipMemcpyAsync(out, f->out4, 4 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

// ---- the map estimate (pk_k_mapsum.hip) ----------------------------
// One shard's moments on the host: h = wsum[2] | mean[L][5] | m2[L][15] | within[L][9] | counts[L].  Reads the particles where they
// are (src[], the adoption buffer): no materialise, no filter state changes -- the colour rows of a table-mode filter are written
// back first, as for a download, and the mode goes on.
static int map_moments_host(pk_filter* f, const char* who, int32_t weighting, double gmax, std::vector<double>& h) {
  if (!f) return fail(PK_ERR_INVALID, "%s: NULL handle", who);
  if (weighting != PK_MAP_UNIFORM && weighting != PK_MAP_WEIGHTED) return fail(PK_ERR_INVALID, "%s: weighting %d", who, weighting);
  if (!f->map_loaded) return fail(PK_ERR_STATE, "%s: no map uploaded", who);
  if (f->dense) return fail(PK_ERR_UNSUPPORTED, "%s: the map estimate reads the compact layout; this filter is on the dense one", who);
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = colour_rows_for_download(f, 0, f->d.P))) return rc;
  const DeviceState& d = f->d;
  const int L = d.lay.L;
  const int Ls = f->grow_on ? f->grow.L0 : L;  // spare slots hold different features in different particles
  const int groups = map_sum_groups(d.P, Ls, f->opt.map_sum_groups);
  const size_t need = map_sum_part_doubles(Ls, groups);
  const size_t head = 2 + 2 * (size_t)kMapSumMaxGroups, n_res = 2 + (size_t)kMapSums * L;
  if ((rc = dev_reserve_group(f, &f->ms_cap, need, need, want(&f->ms_part, need), want(&f->ms_res, head + n_res)))) return rc;
  try {
    h.resize(n_res);
  } catch (const std::bad_alloc&) {
    return fail(PK_ERR_NOMEM, "%s: no host memory for %d landmarks' moments", who, L);
  }
  {
    Span t(f, PK_T_SUMMARY);
    if (weighting == PK_MAP_WEIGHTED && std::isnan(gmax)) {  // this handle's own maximum
      launch_block_max(f->stream, f->d, f->partial, f->ms_res);
      PK_HIP(hipMemcpyAsync(&gmax, f->ms_res, sizeof(double), hipMemcpyDeviceToHost, f->stream));
      PK_HIP(hipStreamSynchronize(f->stream));
    }
    if (weighting == PK_MAP_WEIGHTED && !std::isfinite(gmax))
      return fail(PK_ERR_STATE, "%s: no finite maximum log-weight (%g): every weight is zero, or one is not finite", who, gmax);
    launch_map_moments(f->stream, d, Ls, weighting == PK_MAP_WEIGHTED, gmax, groups, f->ms_part, f->ms_res + 2, f->ms_res + head);
  }
  PK_LAUNCH_CHECK(who);
  PK_HIP(hipMemcpyAsync(h.data(), f->ms_res + head, n_res * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  if (!(h[0] > 0.0) || !std::isfinite(h[0]) || !std::isfinite(h[1]))
    return fail(PK_ERR_STATE, "%s: the weights sum to %g: not positive and finite", who, h[0]);
  return PK_OK;
}

int pk_map_moments(pk_filter* f, int32_t weighting, double gmax, double wsum[2], double* mean, double* m2, double* within, double* counts) {
  std::vector<double> h;
  int rc;
  if ((rc = map_moments_host(f, "pk_map_moments", weighting, gmax, h))) return rc;
  const size_t L = (size_t)f->d.lay.L;
  if (wsum) memcpy(wsum, h.data(), 2 * sizeof(double));
  if (mean) memcpy(mean, h.data() + 2, L * 5 * sizeof(double));
  if (m2) memcpy(m2, h.data() + 2 + L * 5, L * 15 * sizeof(double));
  if (within) memcpy(within, h.data() + 2 + L * 20, L * 9 * sizeof(double));
  if (counts) memcpy(counts, h.data() + 2 + L * 29, L * sizeof(double));
  return PK_OK;
}

int pk_map_summary(pk_filter* f, int32_t weighting, double* mean, double* cov_within, double* cov_between, double* update_count, double* n_eff) {
  std::vector<double> h;
  int rc;
  if ((rc = map_moments_host(f, "pk_map_summary", weighting, std::nan(""), h))) return rc;
  const size_t L = (size_t)f->d.lay.L;
  const double W = h[0];
  if (mean) memcpy(mean, h.data() + 2, L * 5 * sizeof(double));
  for (size_t l = 0; l < L; ++l) {
    const double* m2 = h.data() + 2 + L * 5 + l * 15;
    const double* wi = h.data() + 2 + L * 20 + l * 9;
    if (cov_within) {  // the compact fields back into the dense 5x5 of pk_download_landmarks (a row beyond the estimate: NaN throughout)
      double* c = cov_within + l * 25;
      for (int i = 0; i < 25; ++i) c[i] = std::isnan(wi[0]) ? wi[0] : 0.0;
      c[0] = wi[F_PXX - F_PXX] / W;
      c[1] = c[5] = wi[F_PXY - F_PXX] / W;
      c[6] = wi[F_PYY - F_PXX] / W;
      c[12] = wi[F_CRR - F_PXX] / W;
      c[13] = c[17] = wi[F_CRG - F_PXX] / W;
      c[14] = c[22] = wi[F_CRB - F_PXX] / W;
      c[18] = wi[F_CGG - F_PXX] / W;
      c[19] = c[23] = wi[F_CGB - F_PXX] / W;
      c[24] = wi[F_CBB - F_PXX] / W;
    }
    if (cov_between) {
      double* c = cov_between + l * 25;
      int k = 0;
      for (int i = 0; i < 5; ++i)
        for (int j = i; j < 5; ++j) c[i * 5 + j] = c[j * 5 + i] = m2[k++] / W;
    }
    if (update_count) update_count[l] = h[2 + L * 29 + l] / W;
  }
  if (n_eff) *n_eff = W * W / h[1];
  return PK_OK;
}

int pk_step(pk_filter* f, double v, double w, double dt, const double* z, uint64_t seed, uint64_t draw,
            const double* blobs, int32_t B, const int32_t* ids, double u, int32_t weight_domain) {
  return step_impl(f, StepMotion::twist(v, w, dt), z, seed, draw, blobs, B, ids, u, weight_domain, nullptr);
}

}  // extern "C"

// The body of pk_motion and pk_motion_odom behind their argument checks: `launch` is the one thing that differs.
int motion_impl(pk_filter* f, const char* who, const double* z, const MotionLaunch& launch) {
  int rc;
  if ((rc = use_device(f))) return rc;
  const double* zd = nullptr;
  if (z) {
    // Parity mode: the caller's (pageable) buffer must be consumed before we return.
    PK_HIP(hipMemcpyAsync(f->z_dev, z, (size_t)f->d.P * 3 * sizeof(double), hipMemcpyHostToDevice, f->stream));
    PK_HIP(hipStreamSynchronize(f->stream));
    zd = f->z_dev;
  }
  Span t(f, PK_T_MOTION);
  // a scan staged by pk_stage_scan and not uploaded yet rides in extra workgroups of this launch
  // (what pk_step does; the sharded step stages the next scan before it calls pk_motion)
  pk_filter::Staged& sg = f->staged;
  if (!z && sg.valid && !sg.uploaded && f->opt.upload_kernel) {
    void* dev_view = nullptr;
    if (hipHostGetDevicePointer(&dev_view, sg.st, 0) == hipSuccess && dev_view) {
      launch(nullptr, f->scan_dev, dev_view, sg.lay.upload_bytes);
      f->pose_part_ok = true;
      sg.uploaded = true;
      f->gmax_fused = false;  // the block's control words (running weight maximum) were just overwritten
      if ((rc = note_upload(f, sg.slot))) return rc;
      PK_LAUNCH_CHECK(who);
      return PK_OK;
    }
    (void)hipGetLastError();
  }
  launch(zd, nullptr, nullptr, 0);
  f->pose_part_ok = true;
  PK_LAUNCH_CHECK(who);
  return PK_OK;
}

int step_impl(pk_filter* f, const StepMotion& m, const double* z, uint64_t seed, uint64_t draw, const double* blobs,
              int32_t B, const int32_t* ids, double u, int32_t weight_domain, const double* gate) {
  const bool reset = gate == nullptr;
  auto resample = [&]() {
    return gate ? pk_resample_adaptive(f, u, weight_domain, *gate, nullptr) : pk_resample(f, u, weight_domain, nullptr);  // :137
  };
  int rc;
  if ((rc = ranges_check(f, "pk_step", B))) return rc;  // (armed ranges this step cannot take: refused before anything moves)
  if (f && !ids && B > 0 && (rc = unique_check(f, "pk_step", B))) {  // (unique association's refusals too: the armed ranges go)
    ranges_disarm(f);
    return rc;
  }
  // Throughput mode with ML association: the host half of the scan upload first, then ONE launch
  // for the motion update and the upload of the scan block, then the observe kernels.
  if (f && !f->dense && !f->grow_on && !z && !ids && B > 0 && blobs && f->map_loaded && f->opt.upload_kernel && m.finite()) {
    bool finite = true;
    for (int i = 0; i < 4 * B && finite; ++i) finite = std::isfinite(blobs[i]);
    if (finite && B <= 65535) {
      if ((rc = use_device(f))) return rc;
      RangeScan rs;
      if ((rc = ranges_take(f, "pk_step", B, &rs))) return rc;
      if ((rc = stage_ml_scan(f, blobs, B, &rs))) return rc;
      pk_filter::Staged& sg = f->staged;
      void* dev_view = nullptr;
      if (hipHostGetDevicePointer(&dev_view, sg.st, 0) == hipSuccess && dev_view) {
        {
          Span t(f, PK_T_MOTION);
          if (m.odom)
            launch_motion_odom(f->stream, f->d, m.delta, m.sigma, nullptr, seed, draw, f->scan_dev, dev_view, sg.lay.upload_bytes, f->pose_part);
          else
            launch_motion(f->stream, f->d, m.v, m.w, m.dt, nullptr, seed, draw, 0, f->scan_dev, dev_view, sg.lay.upload_bytes, f->pose_part);
          f->pose_part_ok = true;
        }
        sg.uploaded = true;
        f->gmax_fused = false;
        if ((rc = note_upload(f, sg.slot))) return rc;
        if ((rc = observe_impl(f, staged_blobs(sg), B, nullptr, nullptr, reset))) return rc;  // :73 (reset fused) + :82-124
        return resample();
      }
      (void)hipGetLastError();
    }
  }
  if ((rc = m.odom ? motion_odom_checked(f, m.delta, m.sigma, z, seed, draw) : pk_motion(f, m.v, m.w, m.dt, z, seed, draw))) {  // :75-77
    ranges_disarm(f);
    return rc;
  }
  if ((rc = observe_impl(f, blobs, B, ids, nullptr, reset))) return rc;   // :73 (reset fused) + :82-124
  return resample();
}

extern "C" {

// ---- section 8(f4) on the device: the new-landmark bookkeeping (pk_k_grow.hip) -------
int pk_grow_enable(pk_filter* f, int32_t preset_landmarks, int32_t reading_capacity, double pair_threshold) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_enable: NULL handle");
  const int L = f->d.lay.L;
  if (preset_landmarks < 0 || preset_landmarks >= L)
    return fail(PK_ERR_INVALID, "pk_grow_enable: %d preset landmarks leave no spare slot among the filter's %d", preset_landmarks, L);
  if (reading_capacity < 1 || reading_capacity > 65536) return fail(PK_ERR_INVALID, "pk_grow_enable: reading_capacity %d outside 1..65536", reading_capacity);
  if (!(pair_threshold >= 0.0)) return fail(PK_ERR_INVALID, "pk_grow_enable: pair_threshold %g", pair_threshold);
  if (f->grow_on) return fail(PK_ERR_STATE, "pk_grow_enable: already enabled on this filter");
  if (f->dense)
    return fail(PK_ERR_STATE, "pk_grow_enable: the bookkeeping kernel writes the compact landmark layout; this filter is on the dense one "
                              "(a covariance or Qt that couples position and colour)");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = ct_end(f))) return rc;  // (growing maps: spare slots get colour blocks of their own)
  GrowState& g = f->grow;
  g.L0 = preset_landmarks;
  g.S = L - preset_landmarks;
  g.R = reading_capacity;
  g.pair_threshold = pair_threshold;
  g.cur = 0;
  const size_t P = (size_t)f->d.P;
  for (int i = 0; i < 2; ++i) {
    if ((rc = dev_alloc(f, &g.hyp[i], P * g.R * 8))) return rc;
    if ((rc = dev_alloc(f, &g.cnt[i], P * 4))) return rc;
    if ((rc = dev_alloc(f, &g.slot_id[i], P * g.S))) return rc;
  }
  std::vector<int32_t> c0(P * 4, 0);
  for (size_t p = 0; p < P; ++p) c0[4 * p + 2] = preset_landmarks + 1;  // FilterParticle.next_id (:298)
  PK_HIP(hipMemcpyAsync(g.cnt[0], c0.data(), P * 16, hipMemcpyHostToDevice, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  f->grow_on = true;
  return PK_OK;
}

static int grow_range(pk_filter* f, const char* who, int64_t p0, int64_t p1) {
  if (!f) return fail(PK_ERR_INVALID, "%s: NULL handle", who);
  if (!f->grow_on) return fail(PK_ERR_STATE, "%s: pk_grow_enable was not called on this filter", who);
  if (p0 < 0 || p1 < p0 || p1 > f->d.P) return fail(PK_ERR_INVALID, "%s: particles [%lld, %lld) of %lld", who, (long long)p0, (long long)p1, (long long)f->d.P);
  return use_device(f);
}

int pk_grow_download(pk_filter* f, int64_t p0, int64_t p1, int32_t* counters, double* readings, int32_t* slot_ids) {
  int rc;
  if ((rc = grow_range(f, "pk_grow_download", p0, p1))) return rc;
  const GrowState& g = f->grow;
  const size_t n = (size_t)(p1 - p0);
  if (n == 0) return PK_OK;
  if (counters) PK_HIP(hipMemcpyAsync(counters, g.cnt[g.cur] + 4 * p0, n * 16, hipMemcpyDeviceToHost, f->stream));
  if (readings) PK_HIP(hipMemcpyAsync(readings, g.hyp[g.cur] + (size_t)p0 * g.R * 8, n * g.R * 64, hipMemcpyDeviceToHost, f->stream));
  if (slot_ids) PK_HIP(hipMemcpyAsync(slot_ids, g.slot_id[g.cur] + (size_t)p0 * g.S, n * g.S * 4, hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_grow_upload(pk_filter* f, int64_t p0, int64_t p1, const int32_t* counters, const double* readings, const int32_t* slot_ids) {
  int rc;
  if ((rc = grow_range(f, "pk_grow_upload", p0, p1))) return rc;
  const GrowState& g = f->grow;
  const size_t n = (size_t)(p1 - p0);
  if (n == 0) return PK_OK;
  if (counters)
    for (size_t i = 0; i < n; ++i)
      if (counters[4 * i] < 0 || counters[4 * i] > g.R || counters[4 * i + 1] < 0 || counters[4 * i + 1] > g.S || counters[4 * i + 3] < 0)
        return fail(PK_ERR_INVALID, "pk_grow_upload: particle %lld: %d readings of %d, %d spare slots of %d in use", (long long)(p0 + (int64_t)i),
                    counters[4 * i], g.R, counters[4 * i + 1], g.S);
  if (counters) PK_HIP(hipMemcpyAsync(g.cnt[g.cur] + 4 * p0, counters, n * 16, hipMemcpyHostToDevice, f->stream));
  if (readings) PK_HIP(hipMemcpyAsync(g.hyp[g.cur] + (size_t)p0 * g.R * 8, readings, n * g.R * 64, hipMemcpyHostToDevice, f->stream));
  if (slot_ids) PK_HIP(hipMemcpyAsync(g.slot_id[g.cur] + (size_t)p0 * g.S, slot_ids, n * g.S * 4, hipMemcpyHostToDevice, f->stream));
  if (f->retire.on() && (rc = retire_restart(f, p0, p1))) return rc;  // (pk_grow_retire: what was written is new to the next pass)
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

int pk_grow_shape(const pk_filter* f, int32_t* preset_landmarks, int32_t* spare_slots, int32_t* reading_capacity) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_shape: NULL handle");
  if (preset_landmarks) *preset_landmarks = f->grow_on ? f->grow.L0 : 0;
  if (spare_slots) *spare_slots = f->grow_on ? f->grow.S : 0;
  if (reading_capacity) *reading_capacity = f->grow_on ? f->grow.R : 0;
  return PK_OK;
}

// pk_grow_init: the rule by which the bookkeeping kernel places a new feature, from the next scan on (it keeps no per-particle state)
int pk_grow_init(pk_filter* f, int32_t mode, double min_parallax) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_init: NULL handle");
  if (!f->grow_on) return fail(PK_ERR_STATE, "pk_grow_init: pk_grow_enable was not called on this filter");
  if (mode != PK_GROW_INIT_REFERENCE && mode != PK_GROW_INIT_TRIANGULATED)
    return fail(PK_ERR_INVALID, "pk_grow_init: mode %d is neither PK_GROW_INIT_REFERENCE nor PK_GROW_INIT_TRIANGULATED", mode);
  if (!(min_parallax >= 0.0 && min_parallax <= M_PI / 2))  // (a NaN fails)
    return fail(PK_ERR_INVALID, "pk_grow_init: min_parallax %g outside [0, pi / 2]", min_parallax);
  static_assert(PK_GROW_INIT_REFERENCE == kGrowInitReference && PK_GROW_INIT_TRIANGULATED == kGrowInitTriangulated, "pk_kernels.hpp");
  f->grow_init.mode = mode;
  f->grow_init.min_parallax = min_parallax;
  f->grow_init.sin_min = std::sin(min_parallax);
  return PK_OK;
}

int pk_grow_init_mode(const pk_filter* f, int32_t* mode, double* min_parallax) {
  if (!f) return fail(PK_ERR_INVALID, "pk_grow_init_mode: NULL handle");
  if (mode) *mode = f->grow_init.mode;
  if (min_parallax) *min_parallax = f->grow_init.min_parallax;
  return PK_OK;
}

// ---- probe ------------------------------------------------------------------------------
int pk_probe(int32_t device, const double pose[3], const double mean[5], const double cov[25],
             const double blob[4], const double Qt[16], double* out) {
  if (!pose || !mean || !cov || !blob || !Qt || !out) return fail(PK_ERR_INVALID, "pk_probe: NULL argument");
  int ndev = pk_device_count();
  if (ndev <= 0) return fail(PK_ERR_HIP, "pk_probe: no HIP device visible (the HIP path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(PK_ERR_INVALID, "pk_probe: device %d of %d", device, ndev);
  const int cls = classify_covariance(cov, 0);
  if (cls < 0) return cls;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(Qt[i])) return fail(PK_ERR_INVALID, "pk_probe: Qt is not finite");
  bool dense = cls == 1;
  {
    double scale = 0;
    for (int i = 0; i < 4; ++i) scale = fmax(scale, fabs(Qt[i * 5]));
    for (int j = 1; j < 4; ++j)
      if (fabs(Qt[j]) > 1e-14 * scale || fabs(Qt[j * 4]) > 1e-14 * scale) dense = true;
    for (int i = 1; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j)
        if (fabs(Qt[i * 4 + j] - Qt[j * 4 + i]) > 1e-9 * (scale > 0 ? scale : 1.0)) dense = true;
  }
  PK_HIP(hipSetDevice(device));
  double in[55];
  memcpy(in, pose, 3 * 8);
  memcpy(in + 3, mean, 5 * 8);
  memcpy(in + 8, cov, 25 * 8);
  memcpy(in + 33, blob, 4 * 8);
  memcpy(in + 37, Qt, 16 * 8);
  blob_directions(blob, 1, in + 53);
  double* dev = nullptr;
  PK_HIP(hipMalloc((void**)&dev, (55 + PK_PROBE_LEN) * sizeof(double)));
  hipError_t e = hipMemcpy(dev, in, sizeof(in), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (dense)
      launch_probe_dense(nullptr, dev, dev + 55);  // xy-rgb coupling or a coupled Qt: the dense formulas
    else
      launch_probe(nullptr, dev, dev + 55);
    e = hipMemcpy(out, dev + 55, PK_PROBE_LEN * sizeof(double), hipMemcpyDeviceToHost);
  }
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(PK_ERR_HIP, "pk_probe: %s", hipGetErrorString(e));
  return PK_OK;
}

#ifdef PK_STAMPS
__attribute__((visibility("default"))) int pk_debug_pub_wave_stamps(unsigned long long* out, int reset) {
  pk::debug_read_pub_wave_stamps(out, reset != 0);  // out[8][12]: k_step_pub's sums per wave of the workgroup
  return PK_OK;
}
__attribute__((visibility("default"))) int pk_debug_stamps(unsigned long long* out, int reset) {
  pk::debug_read_stamps(out, reset != 0);            // out[0..15]: k_assoc_grid
  pk::debug_read_fused_stamps(out + 16, reset != 0);  // out[16..31]: k_step_fused
  pk::debug_read_regs_stamps(out + 32, reset != 0);   // out[32..47]: k_step_regs
  pk::debug_read_pub_stamps(out + 48, reset != 0);    // out[48..63]: k_step_pub
  return PK_OK;
}
#endif

// ---- instrumentation ----------------------------------------------------------------------
int pk_enable_timing(pk_filter* f, int32_t on) {
  if (!f) return fail(PK_ERR_INVALID, "pk_enable_timing: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = drain_timings(f))) return rc;
  f->timing_mask = on < 0 ? 0xffffffffu : (uint32_t)on;
  return PK_OK;
}
int pk_reset_timings(pk_filter* f) {
  if (!f) return fail(PK_ERR_INVALID, "pk_reset_timings: NULL handle");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = drain_timings(f))) return rc;
  for (int i = 0; i < PK_T_COUNT; ++i) {
    f->ms[i] = 0;
    f->launches[i] = 0;
    f->timing_seen[i] = 0;
  }
  return PK_OK;
}
int pk_timings(pk_filter* f, double ms[PK_T_COUNT], int64_t launches[PK_T_COUNT]) {
  if (!f || !ms || !launches) return fail(PK_ERR_INVALID, "pk_timings: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  if ((rc = drain_timings(f))) return rc;
  for (int i = 0; i < PK_T_COUNT; ++i) {
    ms[i] = f->ms[i];
    launches[i] = f->launches[i];
  }
  return PK_OK;
}
int pk_download_sources(pk_filter* f, int32_t* src) {
  if (!f || !src) return fail(PK_ERR_INVALID, "pk_download_sources: NULL argument");
  int rc;
  if ((rc = use_device(f))) return rc;
  PK_HIP(hipMemcpyAsync(src, f->d.src[f->d.cur], (size_t)f->d.P * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
  PK_HIP(hipStreamSynchronize(f->stream));
  return PK_OK;
}

}  // extern "C"
