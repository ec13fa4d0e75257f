// Dev probe for profiles/r13_s2d3_nine_tuples.md: does a wave with NINE f32x16 accumulator tuples in architectural registers (no AGPR
// split, operands through a short ring) keep the fp32 matrix pipe as busy as today's eight AGPR tuples, at two waves per SIMD? Same
// skeleton as tools/wino44_issue_probe.hip (8 waves per block, one barrier per step, V through LDS, weights from an L2-resident buffer,
// no data flow that matters); ARCH = 1 drops the "a" constraints and holds the A operands in a ring of RING entries.
//   NM MFMAs (v_mfma_f32_32x32x2_f32 on NACC accumulators) + NV fp32 VALU + NPL b64 pixel loads + NW ds_write_b64 + NRA global b128 +
//   NRB ds_read_b128 per wave and step.
//   S2D = 2 walk as shipped, 128 ch x 32 tiles (average step): NACC 8, NM 12-13 (100 per eight-step body), NV 10, NPL 3, NW 3, NRA 3, NRB 3
//   planned 256 ch x 32 tiles, nine positions per wave:       NACC 9, NM 25 (200 per body),             NV 10, NPL 3, NW 3, NRA 6, NRB 6
// hipcc --offload-arch=gfx950 -O3 tools/wino_s2d3_nine_probe.hip -o tools/wino_s2d3_nine_probe.bin && tools/wino_s2d3_nine_probe.bin
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int ARCH, int RING, int NACC, int NM, int NV, int NPL, int NW, int NRA, int NRB>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k(float* out, const float* wsrc, const float* psrc, int steps, unsigned wbytes, unsigned pbytes) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f32x16 acc[NACC];
  for (int i = 0; i < NACC; ++i) for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NA_ = NRA > 0 ? (ARCH ? RING : NRA) : 1, NB_ = NRB > 0 ? RING : 1, NP_ = NPL > 0 ? 4 : 1;
  f32x4 A[NA_], Bv[NB_];
  f32x2 px[NP_];
  float t[12];
  for (int i = 0; i < 12; ++i) t[i] = lane * 0.25f + i;
  for (int i = 0; i < NA_; ++i) A[i] = (f32x4){1.f, 0.5f, 0.25f, 0.125f};
  for (int i = 0; i < NB_; ++i) Bv[i] = (f32x4){0.3f, 0.2f, 0.1f, 0.05f};
  for (int i = 0; i < NP_; ++i) px[i] = (f32x2){0.f, 0.f};
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)wsrc, 0, (int)wbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)psrc, 0, (int)pbytes, 0x00020000);
  const int vw = lane * 16 + wave * 1024, vp = (threadIdx.x * 8 + blockIdx.x * 4096) & (pbytes - 1);
  const unsigned lw = (threadIdx.x & 511) * 8, lr = (wave & 3) * 9216 + lane * 16;
  for (int s = 0; s < steps; ++s) {
    const int so = (s * 16384) & (wbytes - 1) & ~16383;
#pragma unroll
    for (int u = 0; u < NM; ++u) {
      const int q = u % NACC, e = (u / NACC) & 3;
      const float a = e == 0 ? A[q % NA_].x : e == 1 ? A[q % NA_].y : e == 2 ? A[q % NA_].z : A[q % NA_].w;
      const float b = e == 0 ? Bv[q % NB_].x : e == 1 ? Bv[q % NB_].y : e == 2 ? Bv[q % NB_].z : Bv[q % NB_].w;
      acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[q], 0, 0, 0);
      if (!ARCH) asm volatile("" : "+a"(acc[q]));
#pragma unroll
      for (int n = 0; n < (NV * (u + 1)) / NM - (NV * u) / NM; ++n) {
        const int i = (NV * u) / NM + n;
        t[i % 12] = fmaf(t[(i + 5) % 12], -4.f, t[(i + 7) % 12]);
      }
      if (NPL && (NPL * (u + 1)) / NM != (NPL * u) / NM) {
        const int i = (NPL * u) / NM;
        t[i % 12] += px[i % NP_].x + px[i % NP_].y;
        px[i % NP_] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rp, vp, (s * 64 + i * 4096) & (pbytes - 1) & ~63, 0));
      }
      if (NW && (NW * (u + 1)) / NM != (NW * u) / NM) {
        const int i = (NW * u) / NM;
        f32x2 v; v.x = t[i % 12]; v.y = t[(i + 1) % 12];
        *reinterpret_cast<f32x2*>(smem + ((s & 1) * 36864 + lw + (i % 9) * 4096)) = v;
      }
      if (NRA && (NRA * (u + 1)) / NM != (NRA * u) / NM) {
        const int i = (NRA * u) / NM;
        A[i % NA_] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, vw, so + i * 1024 * 8, 0));
      }
      if (NRB && (NRB * (u + 1)) / NM != (NRB * u) / NM) {
        const int i = (NRB * u) / NM;
        Bv[i % NB_] = *reinterpret_cast<f32x4*>(smem + (((s + 1) & 1) * 36864 + lr + (i % 9) * 1024));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  float sum = 0.f;
  for (int i = 0; i < NACC; ++i) for (int r = 0; r < 16; ++r) sum += acc[i][r];
  for (int i = 0; i < 12; ++i) sum += t[i];
  out[blockIdx.x * 512 + threadIdx.x] = sum;
}

template <int ARCH, int RING, int NACC, int NM, int NV, int NPL, int NW, int NRA, int NRB>
static double run(const char* name, float* out, float* w, float* p, unsigned wb, unsigned pb) {
  const int steps = 2048, grid = 256 * 4;
  hipFuncSetAttribute((const void*)k<ARCH, RING, NACC, NM, NV, NPL, NW, NRA, NRB>, hipFuncAttributeMaxDynamicSharedMemorySize, 73728);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int rep = 0; rep < 2; ++rep) {
    hipEventRecord(e0);
    hipLaunchKernelGGL((k<ARCH, RING, NACC, NM, NV, NPL, NW, NRA, NRB>), dim3(grid), dim3(512), 73728, 0, out, w, p, steps, wb, pb);
    hipEventRecord(e1); hipEventSynchronize(e1);
  }
  float ms; hipEventElapsedTime(&ms, e0, e1);
  if (hipGetLastError() != hipSuccess) { printf("%s: launch failed\n", name); return 0; }
  const double fl = (double)grid * 8 * steps * NM * 4096.0, tf = fl / ms / 1e9;
  printf("%-86s %8.3f ms  %6.1f TF  %.3f of 157.3\n", name, ms, tf, tf / 157.3);
  return tf / 157.3;
}

int main() {
  float *out, *w, *p; const unsigned wb = 1u << 22, pb = 1u << 24;
  hipMalloc(&out, 256 * 4 * 512 * 4); hipMalloc(&w, wb); hipMalloc(&p, pb); hipMemset(w, 0, wb); hipMemset(p, 0, pb);
  const double b8 = run<0, 3, 8, 32, 0, 0, 0, 0, 0>("bare: 32 MFMAs / step on 8 AGPR tuples", out, w, p, wb, pb);
  const double b9 = run<1, 3, 9, 36, 0, 0, 0, 0, 0>("bare: 36 MFMAs / step on 9 architectural tuples", out, w, p, wb, pb);
  run<0, 3, 9, 36, 0, 0, 0, 0, 0>("bare: 36 MFMAs / step on 9 AGPR-pinned tuples (r06's case)", out, w, p, wb, pb);
  run<1, 3, 8, 32, 0, 0, 0, 0, 0>("bare: 32 MFMAs / step on 8 architectural tuples", out, w, p, wb, pb);
  run<0, 3, 8, 32, 16, 4, 4, 8, 8>("stride-1 mix as shipped (8 AGPR): 32 MFMA +16 VALU +4 px +4 dsw +8 A +8 B", out, w, p, wb, pb);
  const double m8a = run<0, 3, 8, 12, 10, 3, 3, 3, 3>("S2D = 2 mix as shipped (8 AGPR), light wave: 12 MFMA +10 VALU +3 px +3 dsw +3 A +3 B", out, w, p, wb, pb);
  const double m8b = run<0, 3, 8, 13, 10, 3, 3, 3, 3>("S2D = 2 mix as shipped (8 AGPR): 13 MFMA +10 VALU +3 px +3 dsw +3 A +3 B", out, w, p, wb, pb);
  const double m9 = run<1, 3, 9, 25, 10, 3, 3, 6, 6>("planned (9 arch, ring 3): 25 MFMA +10 VALU +3 px +3 dsw +6 A +6 B", out, w, p, wb, pb);
  run<1, 4, 9, 25, 10, 3, 3, 6, 6>("planned (9 arch, ring 4): 25 MFMA +10 VALU +3 px +3 dsw +6 A +6 B", out, w, p, wb, pb);
  run<1, 3, 9, 36, 10, 3, 3, 9, 9>("planned, odd-odd step (9 arch, ring 3): 36 MFMA +10 VALU +3 px +3 dsw +9 A +9 B", out, w, p, wb, pb);
  run<1, 3, 9, 16, 8, 2, 2, 4, 4>("planned, even-even step (9 arch, ring 3): 16 MFMA +8 VALU +2 px +2 dsw +4 A +4 B", out, w, p, wb, pb);
  printf("bare nine architectural / bare eight AGPR = %.3f\n", b8 > 0 ? b9 / b8 : 0.);
  printf("planned mix / shipped S2D = 2 mix (12.5 MFMA average) = %.3f\n", (m8a + m8b) > 0 ? m9 / (0.5 * (m8a + m8b)) : 0.);
  return 0;
}
