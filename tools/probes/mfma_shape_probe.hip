// Probe (not product): which bf16 MFMA shape the chip runs faster under its power budget at conv_patch_kernel's
// operating point (lr_conv_patch.hip): one wave per SIMD on 256 workgroups, a 192-register output tile per wave, the A
// operand re-read from LDS with ds_read_b128 at every step, B in registers.  One step is one tap of that kernel
// (96 positions x 64 output channels x 32 input channels per wave): 24 v_mfma_f32_32x32x16_bf16 (6 row tiles x 2 column
// tiles x 2 k chunks) or 48 v_mfma_f32_16x16x32_bf16 (12 row tiles x 4 column tiles), 12 ds_read_b128 and 768 MFMA
// cycles either way.  Reports wall time (events), wave cycles (s_memtime around the loop, median over waves) and the
// clock they imply (s_memtime / s_memrealtime), on random operands and on zeros: on zeros the chip holds its full clock
// and the shapes rank by cycles; on random data the clock it holds decides.
// The 16x16x32 loop issues its MFMAs as asm with the accumulator tied in place, as the kernel does: through the builtin
// hipcc does not keep 48 four-register accumulators where they are over the loop's back edge and copies them through
// VGPRs in every step (200 v_accvgpr_* and 44 s_nop per step), which is not the shape's cost.
//   hipcc -O2 --offload-arch=gfx950 tools/probes/mfma_shape_probe.hip -o /tmp/mfma_shape_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int kSets = 4, kSetBytes = 12 * 1024;   // four sets of 12 A fragments (1 KB per wave read), cycled by step

// stamps[0 .. nwaves): cycles of the loop; stamps[nwaves .. 2 nwaves): 100 MHz ticks of the loop
template <bool S16>
__global__ __launch_bounds__(256, 1) void loop_kernel(const uint4* __restrict__ adata, const uint4* __restrict__ bdata,
                                                      float* sink, unsigned long long* stamps, int iters) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kSets * kSetBytes];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int u = tid; u < kSets * kSetBytes / 16; u += 256) reinterpret_cast<uint4*>(lds)[u] = adata[u];
  bf16x8 b[4];
  for (int q = 0; q < 4; ++q) {
    const uint4 v = bdata[q * 256 + tid];
    b[q] = *reinterpret_cast<const bf16x8*>(&v);
  }
  __syncthreads();
  f32x16 acc32[6][2] = {};
  f32x4 acc16[12][4] = {};
  // A fragments double-buffered per half step (six 1 KB reads fly during the other half's MFMAs), as in the kernel
  bf16x8 a0[6], a1[6];
  auto load_a = [&](bf16x8 (&aa)[6], int it, int half) {
    const unsigned char* p = lds + (it & (kSets - 1)) * kSetBytes + half * 6144 + lane * 16;
#pragma unroll
    for (int m = 0; m < 6; ++m) aa[m] = *reinterpret_cast<const bf16x8*>(p + m * 1024);
  };
  load_a(a0, 0, 0);
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    if constexpr (S16) {
      // written out and pinned, as in the kernel: 12 x {1 LDS read, 4 MFMAs}
      const unsigned char* p0 = lds + (it & (kSets - 1)) * kSetBytes + 6144 + lane * 16;
      const unsigned char* p1 = lds + ((it + 1) & (kSets - 1)) * kSetBytes + lane * 16;
#pragma unroll
      for (int g = 0; g < 12; ++g) {
        const int i = g % 6;
        if (g < 6) a1[i] = *reinterpret_cast<const bf16x8*>(p0 + i * 1024);
        else a0[i] = *reinterpret_cast<const bf16x8*>(p1 + i * 1024);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc16[g][n]) : "v"(g < 6 ? a0[i] : a1[i]), "v"(b[n]));
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      load_a(a1, it, 1);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (half) load_a(a0, it + 1, 0);
#pragma unroll
        for (int kc = 0; kc < 2; ++kc)
#pragma unroll
          for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
              acc32[3 * half + m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16((half ? a1 : a0)[2 * m + kc], b[2 * kc + n],
                                                                               acc32[3 * half + m][n], 0, 0, 0);
      }
      // one LDS read in front of every twelfth of a step's MFMAs, as in the parent kernel
#pragma unroll
      for (int g = 0; g < 12; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
    }
  }
  if constexpr (S16) asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");   // the asm MFMAs retire before their results are read
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float t = 0.f;
  if constexpr (S16) {
    for (int m = 0; m < 12; ++m)
      for (int n = 0; n < 4; ++n)
        for (int i = 0; i < 4; ++i) t += acc16[m][n][i];
  } else {
    for (int m = 0; m < 6; ++m)
      for (int n = 0; n < 2; ++n)
        for (int i = 0; i < 16; ++i) t += acc32[m][n][i];
  }
  if (t == 123.456f) sink[0] = t;
  if (lane == 0) {
    const int w = blockIdx.x * 4 + (tid >> 6), nw = gridDim.x * 4;
    stamps[w] = c1 - c0;
    stamps[nw + w] = r1 - r0;
  }
}

int main() {
  const int nA = kSets * kSetBytes / 2, nB = 4 * 256 * 8, nw = 256 * 4, iters = 20000;
  unsigned short *ad, *bd;
  float* sink;
  unsigned long long* stamps;
  CK(hipMalloc(&ad, nA * 2));
  CK(hipMalloc(&bd, nB * 2));
  CK(hipMalloc(&sink, 4));
  CK(hipMalloc(&stamps, 2 * nw * 8));
  std::vector<unsigned short> ha(nA), hb(nB);
  std::vector<unsigned long long> hs(2 * nw);
  auto launch = [&](int s16) {
    if (s16) hipLaunchKernelGGL(loop_kernel<true>, dim3(256), dim3(256), 0, 0, (const uint4*)ad, (const uint4*)bd, sink, stamps, iters);
    else hipLaunchKernelGGL(loop_kernel<false>, dim3(256), dim3(256), 0, 0, (const uint4*)ad, (const uint4*)bd, sink, stamps, iters);
  };
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int zeros = 0; zeros < 2; ++zeros) {
    // random: bf16 of uniform [-0.5, 0.5) (upper 16 bits of the float)
    auto rnd = [&]() {
      const float f = zeros ? 0.f : (float)(rand() & 0xffff) / 65536.f - 0.5f;
      unsigned u;
      memcpy(&u, &f, 4);
      return (unsigned short)(u >> 16);
    };
    for (auto& v : ha) v = rnd();
    for (auto& v : hb) v = rnd();
    CK(hipMemcpy(ad, ha.data(), nA * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(bd, hb.data(), nB * 2, hipMemcpyHostToDevice));
    for (int i = 0; i < 100; ++i) launch(i & 1);   // ~1 s of back-to-back launches before the first timed one
    CK(hipDeviceSynchronize());
    double wall[2][5], cyc[2][5], ghz[2][5];
    for (int rep = 0; rep < 5; ++rep)
      for (int s16 = 0; s16 < 2; ++s16) {
        launch(s16);   // a launch of this shape in front of the timed one
        CK(hipEventRecord(e0));
        launch(s16);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipMemcpy(hs.data(), stamps, 2 * nw * 8, hipMemcpyDeviceToHost));
        std::vector<double> c(nw), g(nw);
        for (int w = 0; w < nw; ++w) {
          c[w] = (double)hs[w];
          g[w] = (double)hs[w] / (double)hs[nw + w] * 0.1;
        }
        std::nth_element(c.begin(), c.begin() + nw / 2, c.end());
        std::nth_element(g.begin(), g.begin() + nw / 2, g.end());
        wall[s16][rep] = ms;
        cyc[s16][rep] = c[nw / 2];
        ghz[s16][rep] = g[nw / 2];
      }
    for (int s16 = 0; s16 < 2; ++s16) {
      printf("%s %s:", zeros ? "zeros " : "random", s16 ? "16x16x32" : "32x32x16");
      for (int rep = 0; rep < 5; ++rep) printf("  %.3f ms %.0f cyc %.2f GHz", wall[s16][rep], cyc[s16][rep], ghz[s16][rep]);
      std::sort(wall[s16], wall[s16] + 5);
      std::sort(cyc[s16], cyc[s16] + 5);
      const double flops = 2.0 * 96 * 64 * 32 * (double)iters * nw;
      printf("  | median %.3f ms, %.1f cyc/step, %.0f TFLOP/s\n", wall[s16][2], cyc[s16][2] / iters, flops / wall[s16][2] / 1e9);
    }
    printf("%s: 32x32x16 / 16x16x32 wall %.3f, cycles %.3f\n", zeros ? "zeros " : "random", wall[0][2] / wall[1][2], cyc[0][2] / cyc[1][2]);
  }
  return 0;
}
