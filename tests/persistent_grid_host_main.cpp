// Stand-alone check of persistent_grid (parakeet_slam_amd/csrc/pk_kernels.hpp), the one function that sizes the grids of the
// persistent observe kernels: no GPU, no HIP call.  tests/test_persistent_grid_host.py builds it with -fsanitize=address,undefined
// and runs it; it prints "persistent_grid ok" and exits 0, or names the first case that failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../parakeet_slam_amd/csrc/pk_kernels.hpp"

namespace {

// The grid arithmetic as every persistent launcher wrote it out before there was one function (launch_step_regs, launch_step_pub,
// launch_step_pub_big, launch_step_pub_duo), guard and all: -1 stands for "the launcher returned without a launch".
int64_t as_the_launchers_wrote_it(int n_cu, int per_cu, int64_t p0, int64_t p1, int reserve_cus, int64_t P) {
  if (p1 < 0) p1 = P;
  if (P == 0 || p1 <= p0) return -1;
  int64_t grid_n = (int64_t)(n_cu - (reserve_cus > 0 && reserve_cus < n_cu ? reserve_cus : 0)) * per_cu;
  if (grid_n > p1 - p0) grid_n = p1 - p0;
  return grid_n;
}

}  // namespace

int main() {
  long cases = 0;
  for (int n_cu : {1, 8, 256})
    for (int per_cu : {1, 2, 3})
      for (int reserve : {-1, 0, 1, n_cu - 1, n_cu, n_cu + 1})
        for (int64_t P : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)100000}) {
          const int64_t ranges[5][2] = {{0, -1}, {0, P}, {3, 3}, {5, 3}, {P - 1, P}};
          for (const auto& r : ranges) {
            pk::ParticleRange pr;
            pr.p0 = r[0];
            pr.p1 = r[1];
            pr.reserve_cus = reserve;
            const int64_t want = as_the_launchers_wrote_it(n_cu, per_cu, r[0], r[1], reserve, P);
            const int64_t got = pk::persistent_grid(n_cu, per_cu, pr, P);
            ++cases;
            // no launch <=> an empty grid; a launch has at least one workgroup, and never more than particles
            const bool ok = want < 0 ? got == 0 : (got == want && got >= 1 && got <= pr.end(P) - pr.p0);
            if (!ok) {
              std::printf("FAILED n_cu %d per_cu %d reserve %d P %lld range (%lld, %lld): %lld, the launchers had %lld\n", n_cu, per_cu,
                          reserve, (long long)P, (long long)r[0], (long long)r[1], (long long)got, (long long)want);
              return 1;
            }
          }
        }
  // the defaults: every particle, no CU held back
  if (pk::persistent_grid(256, 1, pk::ParticleRange(), 100000) != 256 || pk::persistent_grid(256, 3, pk::ParticleRange(), 500) != 500) {
    std::printf("FAILED default range\n");
    return 1;
  }
  if (cases != 3 * 3 * 6 * 4 * 5) {
    std::printf("FAILED %ld cases\n", cases);
    return 1;
  }
  std::printf("persistent_grid ok\n");
  return 0;
}
