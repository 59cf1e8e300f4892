// Host check of csrc/spectrum.hip (its transform helpers are __host__ __device__ for this): the Stockham passes, run
// thread by thread as the kernel's 256 threads run them, with both forms of the twiddle table, and the two-rows-in-one-
// transform unpacking, against a direct DFT in long double, for widths over every radix mix; the width plan and the slab
// size for unsupported shapes.  Built and run (the host side only) by tests/test_spectrum_cpu.py; exit status 0 = every width within
// 1e-15 in units of sqrt(ref(k) * sum_k ref).
#include "../cra5_amd/csrc/spectrum.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main() {
  const int Ws[] = {2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 25, 30, 45, 96, 240, 360, 720, 1440, 1024, 729, 1125, 1215, 1250, 1280};
  double worst = 0;
  for (int W : Ws) {
    Plan plan;
    if (!make_plan(W, plan)) { printf("no plan for %d\n", W); return 1; }
    std::vector<cplx> tw(W), a(kMaxW), b(kMaxW);
    for (int j = 0; j < W; ++j) tw[j] = {(double)cosl(-2 * M_PIl * j / W), (double)sinl(-2 * M_PIl * j / W)};
    std::vector<double> ra(W), rb(W);
    srand(W);
    for (int j = 0; j < W; ++j) { ra[j] = rand() / (double)RAND_MAX - 0.3; rb[j] = 5 + rand() / (double)RAND_MAX; a[j] = {ra[j], rb[j]}; }
    cplx *in = a.data(), *out = b.data();
    int ns = 1;
    for (int p = 0; p < plan.n; ++p) {
      const int R = plan.radix[p];
      const int half = (W % 2 == 0 && (p & 1)) ? W / 2 : W;   // alternate the two table forms
      for (int tid = 0; tid < 256; ++tid) pass(R, in, out, tw.data(), half, W, ns, tid, 256);
      ns *= R;
      std::swap(in, out);
    }
    if (ns != W) { printf("ns %d != W %d\n", ns, W); return 1; }
    double sa = 0, sb = 0, err = 0;
    std::vector<double> PA(W / 2 + 1), PB(W / 2 + 1), QA(W / 2 + 1), QB(W / 2 + 1);
    for (int k = 0; k <= W / 2; ++k) {
      long double ar = 0, ai = 0, br = 0, bi = 0;
      for (int j = 0; j < W; ++j) {
        long double c = cosl(-2 * M_PIl * (long double)((long long)j * k % W) / W), s = sinl(-2 * M_PIl * (long double)((long long)j * k % W) / W);
        ar += ra[j] * c; ai += ra[j] * s; br += rb[j] * c; bi += rb[j] * s;
      }
      double pa, pb;
      unpack_power(in[k], in[k ? W - k : 0], pa, pb);
      PA[k] = pa / 4; PB[k] = pb / 4; QA[k] = (double)(ar * ar + ai * ai); QB[k] = (double)(br * br + bi * bi);
      sa += QA[k]; sb += QB[k];
    }
    for (int k = 0; k <= W / 2; ++k) {
      err = fmax(err, fabs(PA[k] - QA[k]) / sqrt(QA[k] * sa + 1e-300));
      err = fmax(err, fabs(PB[k] - QB[k]) / sqrt(QB[k] * sb + 1e-300));
    }
    printf("W %4d passes %d err %.3g\n", W, plan.n, err);
    worst = fmax(worst, err);
  }
  Plan p;
  printf("plan(44) %d plan(7) %d plan(1441) %d plan(1) %d slab(268,721,1440) %zu slab44 %zu\n", make_plan(44, p), make_plan(7, p),
         make_plan(1441, p), make_plan(1, p), cra5_zonal_spectrum_slab_bytes(268, 721, 1440), cra5_zonal_spectrum_slab_bytes(1, 4, 44));
  if (make_plan(44, p) || make_plan(7, p) || make_plan(1441, p) || make_plan(1, p) || !make_plan(1215, p)) return 3;
  if (cra5_zonal_spectrum_slab_bytes(1, 4, 44) != 0 || cra5_zonal_spectrum_slab_bytes(268, 721, 1440) == 0) return 4;
  printf("worst %.3g\n", worst);
  return worst < 1e-15 ? 0 : 2;
}
