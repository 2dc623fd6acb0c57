// The math probe (pk_probe_math): the float64 primitives of pk_math.hpp, pk_pub_math.hpp and pk_device.hpp on arrays of
// arguments, one element per thread, so that the tests can hold each of them to an exact reference over its whole domain
// (tests/test_gpu_math_probe.py) -- and the algebra built from them, ekf_update in each of its variants and the match densities
// (tests/test_gpu_ekf_reference.py).  The kernels CALL the functions of the three headers -- nothing is restated here: what is
// measured is what the observe kernels run, inline assembly and all.  Diagnostic only; no kernel of the step is in this file,
// and the entry point lives here beside its kernels.
#include "pk_device.hpp"
#include "pk_filter.hpp"
#include "pk_pub_math.hpp"
#include "pk_range_math.hpp"

namespace pk {

__device__ __forceinline__ double bits_to_double(unsigned long long b) {
  double x;
  memcpy(&x, &b, 8);
  return x;
}

// one landmark from 14 doubles in the compact row order of pk_layout.hpp
__device__ __forceinline__ Landmark<double> landmark_of_row(const double* __restrict__ r, int count) {
  Landmark<double> lm;
  lm.mx = r[F_MX];
  lm.my = r[F_MY];
  lm.mr = r[F_MR];
  lm.mg = r[F_MG];
  lm.mb = r[F_MB];
  lm.pxx = r[F_PXX];
  lm.pxy = r[F_PXY];
  lm.pyy = r[F_PYY];
  lm.crr = r[F_CRR];
  lm.crg = r[F_CRG];
  lm.crb = r[F_CRB];
  lm.cgg = r[F_CGG];
  lm.cgb = r[F_CGB];
  lm.cbb = r[F_CBB];
  lm.count = count;
  return lm;
}
__device__ __forceinline__ void row_of_landmark(const Landmark<double>& lm, double* __restrict__ r) {
  r[F_MX] = lm.mx;
  r[F_MY] = lm.my;
  r[F_MR] = lm.mr;
  r[F_MG] = lm.mg;
  r[F_MB] = lm.mb;
  r[F_PXX] = lm.pxx;
  r[F_PXY] = lm.pxy;
  r[F_PYY] = lm.pyy;
  r[F_CRR] = lm.crr;
  r[F_CRG] = lm.crg;
  r[F_CRB] = lm.crb;
  r[F_CGG] = lm.cgg;
  r[F_CGB] = lm.cgb;
  r[F_CBB] = lm.cbb;
}

constexpr int kEkfIn = 31, kEkfOut = 17, kMatchIn = 23, kMatchOut = 5;

// ekf_update with the expected bearing supplied (KNOWN) or not, the colour block updated (COLOUR) or not, the logarithm of the
// norm left to the caller (FRO) or not
template <bool COLOUR, bool KNOWN, bool FRO>
__device__ __forceinline__ double ekf_variant(Landmark<double>& lm, double sx, double sy, const BlobT<double>& z,
                                              const Noise<double>& qt, bool immutable, double zhat0, double& prod) {
  return ekf_update<double, COLOUR>(lm, sx, sy, z, qt, immutable, nullptr, KNOWN ? &zhat0 : nullptr, FRO ? &prod : nullptr);
}

// in[n][arity(OP)] -> out[n][outputs(OP)], row-major
template <int OP>
__global__ void __launch_bounds__(256) k_probe_math(const double* __restrict__ in, double* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (OP == PK_MATH_LOG_FEW_ULP) {
    out[i] = log_few_ulp(in[i]);
  } else if constexpr (OP == PK_MATH_PUB_LOG) {
    out[i] = pub_log(in[i]);
  } else if constexpr (OP == PK_MATH_PUB_RECIP) {
    out[i] = pub_recip(in[i]);
  } else if constexpr (OP == PK_MATH_ATAN2) {
    out[i] = pk_atan2(in[2 * i], in[2 * i + 1]);
  } else if constexpr (OP == PK_MATH_ROUND_DOWN_F32) {
    out[i] = (double)pub_round_down_to_float(in[i]);
  } else if constexpr (OP == PK_MATH_KEY) {  // both outputs are 64 raw bits
    const unsigned long long k = double_to_key(in[i]);
    out[2 * i] = bits_to_double(k);
    out[2 * i + 1] = key_to_double(k);
  } else if constexpr (OP == PK_MATH_FAR_BOUND) {
    Landmark<double> lm = landmark_of_row(in + (int64_t)F_COUNT_FIELDS * i, 0);
    double fk, fi;
    pub_far_bound(lm, fk, fi);
    out[2 * i] = fk;
    out[2 * i + 1] = fi;
  } else if constexpr (OP == PK_MATH_PR_FROM_PARTS) {
    out[i] = pr_from_parts(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]);
  } else if constexpr (OP == PK_MATH_EKF_UPDATE) {
    // sx sy | 14 fields | count | bearing r g b | q00 rr rg rb gg gb bb | zhat0 | flags | prod_in
    const double* r = in + (int64_t)kEkfIn * i;
    Landmark<double> lm = landmark_of_row(r + 2, (int)r[16]);
    const BlobT<double> z{r[17], r[18], r[19], r[20]};
    const Noise<double> qt = make_noise(r[21], r[22], r[23], r[24], r[25], r[26], r[27]);
    const double zhat0 = r[28];
    const int flags = (int)r[29];  // 1 immutable, 2 zhat0_known, 4 COLOUR = false, 8 fro_prod
    double prod = r[30];
    const bool immutable = (flags & 1) != 0;
    double logw;
    switch ((flags >> 1) & 7) {  // every variant with its pointers known at compile time, as the step kernels call it
      case 0: logw = ekf_variant<true, false, false>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
      case 1: logw = ekf_variant<true, true, false>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
      case 2: logw = ekf_variant<false, false, false>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
      case 3: logw = ekf_variant<false, true, false>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
      case 4: logw = ekf_variant<true, false, true>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
      case 5: logw = ekf_variant<true, true, true>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
      case 6: logw = ekf_variant<false, false, true>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
      default: logw = ekf_variant<false, true, true>(lm, r[0], r[1], z, qt, immutable, zhat0, prod); break;
    }
    double* o = out + (int64_t)kEkfOut * i;  // logw | 14 fields | count | prod
    o[0] = logw;
    row_of_landmark(lm, o + 1);
    o[15] = (double)lm.count;
    o[16] = prod;
  } else {
    static_assert(OP == PK_MATH_MATCH, "unknown op");
    // sx sy heading | 14 fields | bearing r g b | ux uy
    const double* r = in + (int64_t)kMatchIn * i;
    const double sx = r[0], sy = r[1], heading = r[2], ux = r[21], uy = r[22];
    const Landmark<double> lm = landmark_of_row(r + 3, 0);
    const BlobT<double> z{r[17], r[18], r[19], r[20]};
    const double pse = pk_atan2(lm.my - sy, lm.mx - sx);  // as probability_of_match forms it
    double nx, ny;
    closest_point(lm.mx, lm.my, sx, sy, ux, uy, nx, ny);
    double* o = out + (int64_t)kMatchOut * i;  // probability_of_match | position | colour | closest point
    o[0] = probability_of_match(lm, sx, sy, heading, z, ux, uy);
    o[1] = prob_position_match(lm, sx, sy, pse, z.bearing, ux, uy);
    o[2] = prob_color_match(lm, z.r, z.g, z.b);
    o[3] = nx;
    o[4] = ny;
  }
}

// The bearing model's primitives (pk_probe_bearing): what 0 the match probabilities, 1 the update -- the rows of PK_MATH_MATCH and
// of PK_MATH_EKF_UPDATE with the heading behind the pose.
constexpr int kBearingEkfIn = 32;
template <int WHAT>
__global__ void __launch_bounds__(256) k_probe_bearing(const double* __restrict__ in, double* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (WHAT == 0) {
    const double* r = in + (int64_t)kMatchIn * i;
    const double sx = r[0], sy = r[1], heading = r[2];
    const Landmark<double> lm = landmark_of_row(r + 3, 0);
    const BlobT<double> z{r[17], r[18], r[19], r[20]};
    double sn, ch, wx, wy;
    sincos(heading, &sn, &ch);
    rotate_ray(r[21], r[22], ch, sn, wx, wy);
    const double pse = pk_atan2(lm.my - sy, lm.mx - sx);
    double nx, ny;
    closest_point<double, kModelBearing>(lm.mx, lm.my, sx, sy, wx, wy, nx, ny);
    double* o = out + (int64_t)kMatchOut * i;
    o[0] = probability_of_match<double, kModelBearing>(lm, sx, sy, heading, z, wx, wy);
    o[1] = prob_position_match<double, kModelBearing>(lm, sx, sy, pse, z.bearing, wx, wy);
    o[2] = prob_color_match(lm, z.r, z.g, z.b);
    o[3] = nx;
    o[4] = ny;
  } else {
    const double* r = in + (int64_t)kBearingEkfIn * i;
    Landmark<double> lm = landmark_of_row(r + 3, (int)r[17]);
    const BlobT<double> z{r[18], r[19], r[20], r[21]};
    const Noise<double> qt = make_noise(r[22], r[23], r[24], r[25], r[26], r[27], r[28]);
    const double pse = r[29];
    const int flags = (int)r[30];
    const bool immutable = (flags & 1) != 0;
    double logw;
    if (flags & 2)
      logw = ekf_update<double, true, kModelBearing>(lm, r[0], r[1], z, qt, immutable, nullptr, &pse, nullptr, r[2]);
    else
      logw = ekf_update<double, true, kModelBearing>(lm, r[0], r[1], z, qt, immutable, nullptr, nullptr, nullptr, r[2]);
    double* o = out + (int64_t)kEkfOut * i;
    o[0] = logw;
    row_of_landmark(lm, o + 1);
    o[15] = (double)lm.count;
    o[16] = r[31];
  }
}

// Range-bearing blobs (pk_probe_range): the rows of pk_probe_bearing with the blob's range and its variance behind them (and, for
// the match, Qt[0][0], which the measured point's covariance takes).  A NaN range takes the bearing model's functions, as in the kernels.
constexpr int kRangeMatchIn = 26, kRangeEkfIn = 33, kRangeEkfOut = 16;
template <int WHAT>
__global__ void __launch_bounds__(256) k_probe_range(const double* __restrict__ in, double* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (WHAT == 0) {
    const double* r = in + (int64_t)kRangeMatchIn * i;
    const double sx = r[0], sy = r[1], heading = r[2];
    const Landmark<double> lm = landmark_of_row(r + 3, 0);
    const BlobT<double> z{r[17], r[18], r[19], r[20]};
    const BlobRange br{r[23], r[24]};
    const double q00 = r[25];
    double sn, ch, wx, wy;
    sincos(heading, &sn, &ch);
    rotate_ray(r[21], r[22], ch, sn, wx, wy);
    double* o = out + (int64_t)kMatchOut * i;
    if (br.has()) {
      o[0] = probability_of_match_range(lm, sx, sy, heading, z, wx, wy, br.rho, br.qr, q00);
      o[1] = prob_position_match_range(lm, sx, sy, wx, wy, br.rho, br.qr, q00, o + 3);
    } else {
      const double pse = pk_atan2(lm.my - sy, lm.mx - sx);
      o[0] = probability_of_match<double, kModelBearing>(lm, sx, sy, heading, z, wx, wy);
      o[1] = prob_position_match<double, kModelBearing>(lm, sx, sy, pse, z.bearing, wx, wy, o + 3);
    }
    o[2] = prob_color_match(lm, z.r, z.g, z.b);
  } else {
    const double* r = in + (int64_t)kRangeEkfIn * i;
    Landmark<double> lm = landmark_of_row(r + 3, (int)r[17]);
    const BlobT<double> z{r[18], r[19], r[20], r[21]};
    const Noise<double> qt = make_noise(r[22], r[23], r[24], r[25], r[26], r[27], r[28]);
    const double pse = r[29];
    const int flags = (int)r[30];
    const bool immutable = (flags & 1) != 0;
    const BlobRange br{r[31], r[32]};
    const bool known = (flags & 2) != 0;  // (each call with its pointer known at compile time, as the kernels call it)
    double logw;
    if (br.has() && known)
      logw = ekf_update_range(lm, r[0], r[1], r[2], z, br.rho, br.qr, qt, immutable, &pse);
    else if (br.has())
      logw = ekf_update_range(lm, r[0], r[1], r[2], z, br.rho, br.qr, qt, immutable);
    else if (known)
      logw = ekf_update<double, true, kModelBearing>(lm, r[0], r[1], z, qt, immutable, nullptr, &pse, nullptr, r[2]);
    else
      logw = ekf_update<double, true, kModelBearing>(lm, r[0], r[1], z, qt, immutable, nullptr, nullptr, nullptr, r[2]);
    double* o = out + (int64_t)kRangeEkfOut * i;
    o[0] = logw;
    row_of_landmark(lm, o + 1);
    o[15] = (double)lm.count;
  }
}

namespace {

template <int OP>
void launch_one(hipStream_t s, const double* in_dev, double* out_dev, int64_t n) {
  hipLaunchKernelGGL(k_probe_math<OP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in_dev, out_dev, n);
}

// rows of doubles per element, in and out; 0 for an unknown op
int math_probe_arity(int op) {
  switch (op) {
    case PK_MATH_LOG_FEW_ULP:
    case PK_MATH_PUB_LOG:
    case PK_MATH_PUB_RECIP:
    case PK_MATH_ROUND_DOWN_F32:
    case PK_MATH_KEY: return 1;
    case PK_MATH_ATAN2: return 2;
    case PK_MATH_FAR_BOUND: return F_COUNT_FIELDS;
    case PK_MATH_PR_FROM_PARTS: return 4;
    case PK_MATH_EKF_UPDATE: return kEkfIn;
    case PK_MATH_MATCH: return kMatchIn;
    default: return 0;
  }
}
int math_probe_outputs(int op) {
  switch (op) {
    case PK_MATH_KEY:
    case PK_MATH_FAR_BOUND: return 2;
    case PK_MATH_EKF_UPDATE: return kEkfOut;
    case PK_MATH_MATCH: return kMatchOut;
    default: return 1;
  }
}

void launch_probe_math(hipStream_t s, int op, const double* in_dev, double* out_dev, int64_t n) {
  switch (op) {
    case PK_MATH_LOG_FEW_ULP: return launch_one<PK_MATH_LOG_FEW_ULP>(s, in_dev, out_dev, n);
    case PK_MATH_PUB_LOG: return launch_one<PK_MATH_PUB_LOG>(s, in_dev, out_dev, n);
    case PK_MATH_PUB_RECIP: return launch_one<PK_MATH_PUB_RECIP>(s, in_dev, out_dev, n);
    case PK_MATH_ATAN2: return launch_one<PK_MATH_ATAN2>(s, in_dev, out_dev, n);
    case PK_MATH_ROUND_DOWN_F32: return launch_one<PK_MATH_ROUND_DOWN_F32>(s, in_dev, out_dev, n);
    case PK_MATH_KEY: return launch_one<PK_MATH_KEY>(s, in_dev, out_dev, n);
    case PK_MATH_FAR_BOUND: return launch_one<PK_MATH_FAR_BOUND>(s, in_dev, out_dev, n);
    case PK_MATH_PR_FROM_PARTS: return launch_one<PK_MATH_PR_FROM_PARTS>(s, in_dev, out_dev, n);
    case PK_MATH_EKF_UPDATE: return launch_one<PK_MATH_EKF_UPDATE>(s, in_dev, out_dev, n);
    case PK_MATH_MATCH: return launch_one<PK_MATH_MATCH>(s, in_dev, out_dev, n);
    default: return;
  }
}

}  // namespace

}  // namespace pk

extern "C" int pk_probe_math(int32_t device, int32_t op, int64_t n, const double* in, double* out) {
  if (!in || !out) return fail(PK_ERR_INVALID, "pk_probe_math: NULL argument");
  const int arity = math_probe_arity(op);
  if (arity == 0) return fail(PK_ERR_INVALID, "pk_probe_math: unknown op %d", op);
  if (n < 0 || n > 2147483647LL) return fail(PK_ERR_INVALID, "pk_probe_math: n = %lld out of range", (long long)n);
  int ndev = pk_device_count();
  if (ndev <= 0) return fail(PK_ERR_HIP, "pk_probe_math: no HIP device visible (the HIP path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(PK_ERR_INVALID, "pk_probe_math: device %d of %d", device, ndev);
  if (n == 0) return PK_OK;
  PK_HIP(hipSetDevice(device));
  const size_t n_in = (size_t)n * arity, n_out = (size_t)n * math_probe_outputs(op);
  double* dev = nullptr;
  PK_HIP(hipMalloc((void**)&dev, (n_in + n_out) * sizeof(double)));
  hipError_t e = hipMemcpy(dev, in, n_in * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_probe_math(nullptr, op, dev, dev + n_in, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dev + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(PK_ERR_HIP, "pk_probe_math: %s", hipGetErrorString(e));
  return PK_OK;
}

extern "C" int pk_probe_bearing(int32_t device, int32_t what, int64_t n, const double* in, double* out) {
  if (!in || !out) return fail(PK_ERR_INVALID, "pk_probe_bearing: NULL argument");
  if (what != 0 && what != 1) return fail(PK_ERR_INVALID, "pk_probe_bearing: what = %d is neither 0 (the match probabilities) nor 1 (the update)", what);
  if (n < 0 || n > 2147483647LL) return fail(PK_ERR_INVALID, "pk_probe_bearing: n = %lld out of range", (long long)n);
  const int arity = what == 0 ? pk::kMatchIn : pk::kBearingEkfIn, outputs = what == 0 ? pk::kMatchOut : pk::kEkfOut;
  if (what == 1)
    for (int64_t i = 0; i < n; ++i) {
      const double fl = in[(size_t)i * arity + 30];
      if (!(fl == 0.0 || fl == 1.0 || fl == 2.0 || fl == 3.0))
        return fail(PK_ERR_INVALID, "pk_probe_bearing: row %lld: flags take bit 0 (immutable) and bit 1 (zhat0 known) only", (long long)i);
    }
  int ndev = pk_device_count();
  if (ndev <= 0) return fail(PK_ERR_HIP, "pk_probe_bearing: no HIP device visible (the HIP path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(PK_ERR_INVALID, "pk_probe_bearing: device %d of %d", device, ndev);
  if (n == 0) return PK_OK;
  PK_HIP(hipSetDevice(device));
  const size_t n_in = (size_t)n * arity, n_out = (size_t)n * outputs;
  double* dev = nullptr;
  PK_HIP(hipMalloc((void**)&dev, (n_in + n_out) * sizeof(double)));
  hipError_t e = hipMemcpy(dev, in, n_in * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (what == 0)
      hipLaunchKernelGGL(pk::k_probe_bearing<0>, grid, dim3(256), 0, nullptr, dev, dev + n_in, n);
    else
      hipLaunchKernelGGL(pk::k_probe_bearing<1>, grid, dim3(256), 0, nullptr, dev, dev + n_in, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dev + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(PK_ERR_HIP, "pk_probe_bearing: %s", hipGetErrorString(e));
  return PK_OK;
}

extern "C" int pk_probe_range(int32_t device, int32_t what, int64_t n, const double* in, double* out) {
  if (!in || !out) return fail(PK_ERR_INVALID, "pk_probe_range: NULL argument");
  if (what != 0 && what != 1) return fail(PK_ERR_INVALID, "pk_probe_range: what = %d is neither 0 (the match probabilities) nor 1 (the update)", what);
  if (n < 0 || n > 2147483647LL) return fail(PK_ERR_INVALID, "pk_probe_range: n = %lld out of range", (long long)n);
  const int arity = what == 0 ? pk::kRangeMatchIn : pk::kRangeEkfIn, outputs = what == 0 ? pk::kMatchOut : pk::kRangeEkfOut;
  if (what == 1)
    for (int64_t i = 0; i < n; ++i) {
      const double fl = in[(size_t)i * arity + 30];
      if (!(fl == 0.0 || fl == 1.0 || fl == 2.0 || fl == 3.0))
        return fail(PK_ERR_INVALID, "pk_probe_range: row %lld: flags take bit 0 (immutable) and bit 1 (zhat0 known) only", (long long)i);
    }
  int ndev = pk_device_count();
  if (ndev <= 0) return fail(PK_ERR_HIP, "pk_probe_range: no HIP device visible (the HIP path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(PK_ERR_INVALID, "pk_probe_range: device %d of %d", device, ndev);
  if (n == 0) return PK_OK;
  PK_HIP(hipSetDevice(device));
  const size_t n_in = (size_t)n * arity, n_out = (size_t)n * outputs;
  double* dev = nullptr;
  PK_HIP(hipMalloc((void**)&dev, (n_in + n_out) * sizeof(double)));
  hipError_t e = hipMemcpy(dev, in, n_in * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (what == 0)
      hipLaunchKernelGGL(pk::k_probe_range<0>, grid, dim3(256), 0, nullptr, dev, dev + n_in, n);
    else
      hipLaunchKernelGGL(pk::k_probe_range<1>, grid, dim3(256), 0, nullptr, dev, dev + n_in, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dev + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(PK_ERR_HIP, "pk_probe_range: %s", hipGetErrorString(e));
  return PK_OK;
}
