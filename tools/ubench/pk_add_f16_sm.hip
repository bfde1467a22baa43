// Does v_pk_add_f16 with a negated second source turn two zero-extended bytes into sign-magnitude?  A half 0x00bb is the f16
// denormal bb * 2^-24; a - r of two such halves is exact, bit 15 = (a < r), bits 7..0 = |a - r|, a == r gives +0.
// Checks all 65 536 (a, r) byte pairs in both halves (the other half holds a different pair) against the integer form and
// checks the v_perm_b32 selectors that gather the four sign bits as bytes, and
// times the instruction on denormal operands next to the plain ops it competes with (issue rate per SIMD).
// Build: hipcc --offload-arch=gfx950 -O3 pk_add_f16_sm.hip -o pk_add_f16_sm.bin ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
__host__ __device__ static uint32_t sm_ref(uint32_t a, uint32_t r) { return (a < r ? 0x8000u : 0u) | (a < r ? r - a : a - r); }
__global__ void check(uint32_t *bad)
{
  const uint32_t a = blockIdx.x, r = threadIdx.x;         /* the pair under test */
  const uint32_t a2 = (a * 7u + 3u) & 0xffu, r2 = 255u - r; /* its neighbour in the other half */
  const uint32_t x = a | (a2 << 16), y = r | (r2 << 16), xs = a2 | (a << 16), ys = r2 | (r << 16);
  uint32_t d, ds;
  asm volatile("v_pk_add_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(x), "v"(y));
  asm volatile("v_pk_add_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(ds) : "v"(xs), "v"(ys));
  const uint32_t e = sm_ref(a, r) | (sm_ref(a2, r2) << 16), es = sm_ref(a2, r2) | (sm_ref(a, r) << 16);
  if (d != e) atomicAdd(&bad[0], 1u);
  if (ds != es) atomicAdd(&bad[1], 1u);
  // the decoder's sign gather: v_perm_b32 selectors 8 .. 11 spread bit 15 / 31 of the second / first source over a byte
  const uint32_t g = __builtin_amdgcn_perm(ds, d, 0x0b090a08u);
  const uint32_t n0 = a < r ? 0xffu : 0u, n1 = a2 < r2 ? 0xffu : 0u; /* d = (pair, neighbour), ds = (neighbour, pair) */
  if (g != (n0 | (n1 << 8) | (n1 << 16) | (n0 << 24))) atomicAdd(&bad[2], 1u);
}
#define N_ACC 16
#define ITERS 1024
// the accumulators start as zero-extended bytes, i.e. the f16 chains run on denormals
#define OPK(NAME, ASMSTR)                                                                              \
  __global__ void __launch_bounds__(256) k_##NAME(uint32_t *out, uint32_t seed)                        \
  {                                                                                                    \
    uint32_t acc[N_ACC];                                                                               \
    for (int i = 0; i < N_ACC; i++) acc[i] = (seed * (i + 1) + threadIdx.x) & 0x00ff00ffu;             \
    for (int it = 0; it < ITERS; it++) {                                                               \
      _Pragma("unroll") for (int i = 0; i < N_ACC; i++)                                                \
        asm volatile(ASMSTR : "=v"(acc[i]) : "v"(acc[i]), "v"(acc[(i + 5) % N_ACC]));                 \
    }                                                                                                  \
    uint32_t r = 0;                                                                                    \
    for (int i = 0; i < N_ACC; i++) r ^= acc[i];                                                       \
    if (r == 0x12345678u) out[0] = r;                                                                  \
  }
OPK(xor_b32, "v_xor_b32 %0, %1, %2")
OPK(or_b32, "v_or_b32 %0, %1, %2")
OPK(sub_u32, "v_sub_u32 %0, %1, %2")
OPK(pk_max_u16, "v_pk_max_u16 %0, %1, %2")
OPK(perm_b32, "v_perm_b32 %0, %1, %2, %2")
OPK(pk_add_f16, "v_pk_add_f16 %0, %1, %2")
OPK(pk_add_f16_neg, "v_pk_add_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]")
typedef void (*kern_t)(uint32_t *, uint32_t);
static void run(const char *name, kern_t kf, uint32_t *d)
{
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const int grid = 256 * 8;
  hipLaunchKernelGGL(kf, dim3(grid), dim3(256), 0, 0, d, 3u);
  (void)hipEventRecord(e0);
  for (int r = 0; r < 5; r++) hipLaunchKernelGGL(kf, dim3(grid), dim3(256), 0, 0, d, 3u + r);
  (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
  float ms; (void)hipEventElapsedTime(&ms, e0, e1); ms /= 5;
  const double wi_per_simd = (double)grid * 4 / (256.0 * 4) * ITERS * N_ACC;
  printf("%-22s %.3f ms  %.3f ns/wave-instr/SIMD\n", name, ms, ms * 1e6 / wi_per_simd);
}
int main()
{
  uint32_t *bad;
  (void)hipMalloc(&bad, 64); (void)hipMemset(bad, 0, 64);
  hipLaunchKernelGGL(check, dim3(256), dim3(256), 0, 0, bad);
  uint32_t hb[3]; (void)hipMemcpy(hb, bad, 12, hipMemcpyDeviceToHost);
  printf("v_pk_add_f16 neg src1 vs integer sign-magnitude, 65536 byte pairs: mismatches low half %u, high half %u\n", hb[0], hb[1]);
  printf("v_perm_b32 0x0b090a08 sign bytes of the four halves: mismatches %u\n", hb[2]);
  run("v_xor_b32", k_xor_b32, bad); run("v_or_b32", k_or_b32, bad); run("v_sub_u32", k_sub_u32, bad);
  run("v_pk_max_u16", k_pk_max_u16, bad); run("v_perm_b32", k_perm_b32, bad);
  run("v_pk_add_f16", k_pk_add_f16, bad); run("v_pk_add_f16 neg", k_pk_add_f16_neg, bad);
  return (hb[0] | hb[1] | hb[2]) ? 1 : 0;
}
