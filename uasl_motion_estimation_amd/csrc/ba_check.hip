// ba_check.hip — the per-landmark residual check behind a BA solve
// (me_ba_point_check, include/me_hip.h): one read-only kernel
// over a plan's CSR by point, in a translation unit of its own so that
// ba.hip's device code is untouched by it.  Of the BA parts it reads the
// types (ba_types.hpp) and one observation's residual (ba_residual.hpp) only.
#include <cmath>
#include "me_internal.hpp"
#include "ba_types.hpp"
#include "ba_residual.hpp"

using namespace ba;

namespace {

// kCheckLanes lanes per landmark, 32 landmarks per workgroup.  A VO window's
// tracks hold at most W observations (2 W in the mono model), mostly a few:
// eight lanes keep the sin / cos chain of rotate() to one or two rounds per
// lane, a whole wave per landmark would idle 56 lanes on the common track.
constexpr int kCheckBlock = 256;
constexpr int kCheckLanes = 8;
static_assert(64 % kCheckLanes == 0, "a landmark's lane group lies inside one wave");

// Per landmark j over its slots of the plan's CSR by point (Bufs::p_off /
// p_obs): chi2 = max over its observations of s_o = ((r0 r0 + r1 r1) + r2 r2)
// + r3 r3 (cost_kernel's sum without the Huber corrector; a non-finite s_o is
// +inf, no observation gives 0), flags bit 0 = !(chi2 <= chi2_max), bit 1 =
// some observation with !(Z_o > z_min), Z_o the camera-frame depth.  A maximum
// and an "any": the same bits whatever the order of the observation arrays,
// without atomics and without initialising the outputs.  A plan whose input
// failed the index validation (State::bad_input) has no CSR to walk: every
// landmark then gets +inf and both bits.
template <int OD>
__global__ __launch_bounds__(kCheckBlock) void point_check_kernel(Geo g, Bufs b, const double* cams, const double* pts,
                                                                  double chi2_max, double z_min, double* chi2,
                                                                  uint8_t* flags) {
  const int j = blockIdx.x * (kCheckBlock / kCheckLanes) + threadIdx.x / kCheckLanes;
  const int l = threadIdx.x % kCheckLanes;
  const bool bad = b.st->bad_input != 0;
  const bool walk = j < g.np && !bad;
  double m = bad ? INFINITY : 0.0;
  int behind = bad ? 1 : 0;
  if (walk) {
    const double* X = pts + 3 * (long)j;
    const int end = b.p_off[j + 1];
    for (int q = b.p_off[j] + l; q < end; q += kCheckLanes) {
      const int o = b.p_obs[q];
      const double* cam = cams + 6 * (long)b.cam_idx[o];
      double r[4], P[3];
      obs_residual<OD>(g, b, o, cam, X, r, nullptr, nullptr);
      // The depth is the residual's own P[2] + cam[2], which obs_residual does not hand out: rotate() again on the
      // same operands.  It is a pure function under -ffp-contract=off, so the bits are the residual's whether or
      // not the compiler merges the two inlined calls; only the cost of a second sin / cos chain rests on that
      // merge (ba_residual.hpp is left as ba.hip builds it, so no variant there returns Z).
      rotate(cam + 3, X, P, nullptr, nullptr);
      const double Z = P[2] + cam[2];
      double s = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3];
      if (!(s <= 1.7976931348623157e308)) s = INFINITY;  // NaN and +inf alike
      m = s > m ? s : m;
      behind |= !(Z > z_min) ? 1 : 0;
    }
  }
  // (every lane of the wave arrives here: the groups' loops have rejoined)
  for (int off = kCheckLanes / 2; off > 0; off >>= 1) {
    const double mo = __shfl_xor(m, off, 64);
    const int bo = __shfl_xor(behind, off, 64);
    m = mo > m ? mo : m;
    behind |= bo;
  }
  if (j < g.np && l == 0) {
    if (chi2) chi2[j] = m;
    flags[j] = (uint8_t)((!(m <= chi2_max) ? 1 : 0) | (behind ? 2 : 0));
  }
}

}  // namespace

const char* me_ba_point_check_check(const me_ba_point_check_params* p) {
  if (!p) return "null parameters";
  if (!(p->chi2_max > 0.0)) return "chi2_max must be > 0 (+inf allowed)";  // (false for NaN)
  if (!(std::isfinite(p->z_min) && p->z_min >= 0.0)) return "z_min must be finite and >= 0";
  return nullptr;
}

extern "C" void me_ba_point_check_default_params(me_ba_point_check_params* p) {
  if (!p) return;
  p->chi2_max = 18.47;  // the 99.9 % point of chi-square with 4 degrees of freedom
  p->z_min = 0.0;
}

int me_ba_check_launch(me_ctx* c, const Geo& g, const Bufs& b, const double* cams, const double* pts,
                       const me_ba_point_check_params* p, double* chi2, uint8_t* flags) {
  if (g.np <= 0) return ME_OK;
  const int nb = (g.np + kCheckBlock / kCheckLanes - 1) / (kCheckBlock / kCheckLanes);
  {
    me_ktimer t(c, ME_KT_BA_CHECK);
    if (g.od == 4)
      hipLaunchKernelGGL(point_check_kernel<4>, dim3(nb), dim3(kCheckBlock), 0, c->stream, g, b, cams, pts, p->chi2_max,
                         p->z_min, chi2, flags);
    else
      hipLaunchKernelGGL(point_check_kernel<2>, dim3(nb), dim3(kCheckBlock), 0, c->stream, g, b, cams, pts, p->chi2_max,
                         p->z_min, chi2, flags);
  }
  return me_check_launch(c, "point_check_kernel");
}
