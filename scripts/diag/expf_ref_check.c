// Exhaustive check of the expf_ref restatement (kernels/expf_ref.h) against
// the host libm expf over every float in [-104, 0]: gcc -O2
// -ffp-contract=off expf_ref_check.c -lm && ./a.out  (glibc 2.35: 1 of 1.1e9
// differs, at x = -63.1).  FIX=i D=d perturbs table entry i (diagnostics).
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
static uint64_t T[32];
static double asd(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint64_t asu(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static float my_expf(float x) {
  const double N = 32.0;
  const double InvLn2N = 0x1.71547652b82fep+0 * N;
  const double SHIFT = 0x1.8p+52;
  const double C0 = 0x1.c6af84b912394p-5 / N / N / N, C1 = 0x1.ebfce50fac4f3p-3 / N / N,
               C2 = 0x1.62e42ff0c52d6p-1 / N;
  double xd = (double)x;
  double z = InvLn2N * xd;
  double kd = z + SHIFT;
  uint64_t ki = asu(kd);
  kd -= SHIFT;
  double r = z - kd;
  uint64_t t = T[ki % 32];
  t += ki << (52 - 5);
  double s = asd(t);
  z = fma(C0, r, C1);
  double r2 = r * r;
  double y = fma(C2, r, 1.0);
  y = fma(z, r2, y);
  y = y * s;
  return (float)y;
}
int main() {
  for (int i = 0; i < 32; ++i) T[i] = asu(exp2((double)i / 32)) - ((uint64_t)i << 47);
  if (getenv("FIX")) { int j = atoi(getenv("FIX")); T[j] += atoi(getenv("D")); }
  long n = 0, diff = 0;
  for (uint32_t b = 0x80000000u; ; ++b) {
    float x; memcpy(&x, &b, 4);
    if (!(x >= -104.0f)) break;
    float a = expf(x), c = my_expf(x);
    n++; if (a != c) { if (diff < 5) printf("x=%.9g expf=%.9g mine=%.9g\n", x, a, c); diff++; }
  }
  printf("n=%ld diff=%ld\n", n, diff);
  for (int i = 0; i < 4; ++i) printf("T[%d]=0x%016llx\n", i, (unsigned long long)T[i]);
}
