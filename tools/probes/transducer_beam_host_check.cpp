// The host side of lr_rnnt_beam_decode under a sanitizer, without a GPU: the size queries over their whole argument range
// and every rejection that answers before a launch.  A stand-alone program (nothing is loaded into Python):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     tools/probes/transducer_beam_host_check.cpp lipreading_amd/csrc/lr_transducer_beam.hip -o beam_host_check
//   ./beam_host_check
#include <cstdio>
#include <cstdlib>

#include "../../include/lipreading_hip.h"

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

int main() {
  // the size queries: 0 outside the limits, the documented sum inside, no overflow at the corners
  for (int B : {-1, 0, 1, 3, 65535, 65536})
    for (int W : {-1, 0, 1, 4, 32, 33})
      for (int M : {-1, 0, 1, 18, 256, 257}) {
        const size_t got = lr_rnnt_beam_state_bytes(B, W, M);
        const bool in = B >= 1 && B <= 65535 && W >= 1 && W <= 32 && M >= 1 && M <= 256;
        const size_t bw = in ? (size_t)B * W : 0;
        EXPECT(got == (in ? 32 + bw * 8 + (size_t)B * 4 + bw * 4 + 2 * bw * M * 4 : 0));
      }
  EXPECT(lr_rnnt_beam_state_bytes(65535, 32, 256) > ((size_t)1 << 32));
  for (int B : {0, 1, 65535, 65536})
    for (int V1 : {1, 2, 37, 256, 257})
      for (int J : {0, 1, 45, 512, 513})
        for (int W : {0, 1, 32, 33})
          for (int S : {0, 1, 8, 9}) {
            const size_t got = lr_rnnt_beam_workspace_bytes(B, V1, J, W, S);
            const bool in = B >= 1 && B <= 65535 && V1 >= 2 && V1 <= 256 && J >= 1 && J <= 512 && W >= 1 && W <= 32 &&
                            S >= 1 && S <= 8;
            if (!in) {
              EXPECT(got == 0);
              continue;
            }
            const size_t V1p = (V1 + 31) / 32 * 32, Jp = (J + 31) / 32 * 32;
            EXPECT(got == V1p * Jp * 4 + (size_t)B * W * 256 * 4 && got % 16 == 0);
          }

  // the rejections: host memory stands in for the device's, nothing is launched
  const int B = 2, T = 3, V1 = 5, J = 8, W = 4, S = 2, M = 6;
  const size_t sb = lr_rnnt_beam_state_bytes(B, W, M), wb = lr_rnnt_beam_workspace_bytes(B, V1, J, W, S);
  void* state = std::aligned_alloc(16, (sb + 15) / 16 * 16);
  void* ws = std::aligned_alloc(16, wb);
  float f[1] = {0.f};
  int32_t i32[1] = {0};
  auto call = [&](const float* e, void* st, size_t st_bytes, void* w, size_t w_bytes, int b, int t, int v1, int j,
                  int ctx, int width, int syms, int nbest, int max_out) {
    return lr_rnnt_beam_decode(e, 0, 0, nullptr, f, f, f, f, st, st_bytes, 1, nullptr, i32, i32, i32, f, i32, i32, w,
                               w_bytes, b, t, v1, j, ctx, width, syms, nbest, max_out, nullptr);
  };
  EXPECT(call(nullptr, state, sb, ws, wb, B, T, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, nullptr, sb, ws, wb, B, T, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, nullptr, wb, B, T, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, 0, T, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, 0, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, 1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 0, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 3, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, 0, S, 1, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W, 0, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W, S, 0, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W, S, W + 1, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W, S, W, 0) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb, 65536, T, V1, J, 2, W, S, W, M) == LR_ERR_UNSUPPORTED);
  EXPECT(call(f, state, sb, ws, wb, B, 4097, V1, J, 2, W, S, W, M) == LR_ERR_UNSUPPORTED);
  EXPECT(call(f, state, sb, ws, wb, B, T, 257, J, 2, W, S, W, M) == LR_ERR_UNSUPPORTED);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, 513, 2, W, S, W, M) == LR_ERR_UNSUPPORTED);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, 33, S, W, M) == LR_ERR_UNSUPPORTED);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W, 9, W, M) == LR_ERR_UNSUPPORTED);
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W, S, W, 257) == LR_ERR_UNSUPPORTED);
  EXPECT(call(f, state, sb - 4, ws, wb, B, T, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);   // a state of another size
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W, S, W, M + 1) == LR_ERR_INVALID_ARG);   // ... of another max_out
  EXPECT(call(f, state, sb, ws, wb, B, T, V1, J, 2, W - 1, S, 1, M) == LR_ERR_INVALID_ARG);   // ... of another width
  EXPECT(call(f, (char*)state + 4, sb, ws, wb, B, T, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, (char*)ws + 4, wb, B, T, V1, J, 2, W, S, W, M) == LR_ERR_INVALID_ARG);
  EXPECT(call(f, state, sb, ws, wb - 1, B, T, V1, J, 2, W, S, W, M) == LR_ERR_WORKSPACE);
  std::free(state);
  std::free(ws);
  std::printf(failures ? "%d checks failed\n" : "transducer beam host checks passed\n", failures);
  return failures ? 1 : 0;
}
