// scripts/conv_launch_log.cc -- what the convolution dispatch would launch,
// without a GPU.  Loads the libkcnn.so given as argv[1], calls every
// hipF_conv2d* entry point over a sweep of geometries (row counts, aligned
// and unaligned operands, with and without workspace, argument errors) and
// prints each return code, workspace size and kernel launch (kernel handle
// offset, grid, block, dynamic LDS bytes).  No kernel runs: hipLaunchKernel,
// the call-configuration pair and the few device calls the host code makes
// are defined in launch_log.h and take precedence over the runtime's.  The
// KCNN_*_X6 environment variables select the kernel families.  Arguments after the
// library replace the built-in sweep by a list of geometries, each
// "H,W,C,kh,kw,G,pad_h,pad_w[,rows]" (9 rows when left out); "-" reads them
// from standard input, one per line (tests/test_conv_routes.py pins the
// routes of single shapes this way).  Two builds dispatch
// alike when their logs are equal after scripts/conv_launch_names.py has
// replaced the handle offsets by symbol names (profiles/conv_dispatch.md):
//   g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       scripts/conv_launch_log.cc -o conv_launch_log -rdynamic -ldl
//   ./conv_launch_log kaldi-cnn_amd/libkcnn.so > new.raw
//   ./conv_launch_log kaldi-cnn_amd/libkcnn.so 20,13,8,3,1,32,0,0 40,61,1,8,3,256,0,0,5
//   python scripts/conv_launch_names.py kaldi-cnn_amd/libkcnn.so new.raw > new.txt
#include <string.h>

#include <vector>

#include "cnsl-hip-kernels.h"
#include "launch_log.h"  // hipLaunchKernel and friends, g_lib, sym

static MatrixDim md(int r, int c, int s = -1) { return MatrixDim{r, c, s < 0 ? c : s}; }

// a geometry (H, W, C, kh, kw, G, pad_h, pad_w) and the row counts to run it at
struct Job {
  int s[8];
  std::vector<int> rows;
};

// "H,W,C,kh,kw,G,pad_h,pad_w[,rows]" (blanks also separate)
static bool parse_job(const char *txt, Job &j) {
  int *s = j.s, R = 9;
  const int n = sscanf(txt, "%d%*[, ]%d%*[, ]%d%*[, ]%d%*[, ]%d%*[, ]%d%*[, ]%d%*[, ]%d%*[, ]%d",
                       s, s + 1, s + 2, s + 3, s + 4, s + 5, s + 6, s + 7, &R);
  j.rows = {R};
  if (n < 8) fprintf(stderr, "bad shape: %s\n", txt);
  return n >= 8;
}

int main(int argc, char **argv) {
  setvbuf(stdout, nullptr, _IONBF, 0);
  if (argc < 2) {
    fprintf(stderr, "usage: %s libkcnn.so [H,W,C,kh,kw,G,pad_h,pad_w[,rows] ... | -]\n", argv[0]);
    return 2;
  }
  open_lib(argv[1]);
  auto conv2d = sym<decltype(&hipF_conv2d)>("hipF_conv2d");
  auto relu = sym<decltype(&hipF_conv2d_relu)>("hipF_conv2d_relu");
  auto maxpool = sym<decltype(&hipF_conv2d_maxpool)>("hipF_conv2d_maxpool");
  auto maxpool3d = sym<decltype(&hipF_conv2d_maxpool3d)>("hipF_conv2d_maxpool3d");
  auto wgrad = sym<decltype(&hipF_conv2d_wgrad)>("hipF_conv2d_wgrad");
  auto dgrad = sym<decltype(&hipF_conv2d_dgrad)>("hipF_conv2d_dgrad");
  auto backward = sym<decltype(&hipF_conv2d_backward)>("hipF_conv2d_backward");
  auto bpool = sym<decltype(&hipF_conv2d_backward_pooled)>("hipF_conv2d_backward_pooled");
  auto bpool3 = sym<decltype(&hipF_conv2d_backward_pooled3d)>("hipF_conv2d_backward_pooled3d");
  auto ws_f = sym<decltype(&hipF_conv2d_workspace_bytes)>("hipF_conv2d_workspace_bytes");
  auto ws_w = sym<decltype(&hipF_conv2d_wgrad_workspace_bytes)>("hipF_conv2d_wgrad_workspace_bytes");
  auto ws_d = sym<decltype(&hipF_conv2d_dgrad_workspace_bytes)>("hipF_conv2d_dgrad_workspace_bytes");
  auto ws_b = sym<decltype(&hipF_conv2d_backward_workspace_bytes)>("hipF_conv2d_backward_workspace_bytes");

  // fake device pointers (never dereferenced on the host)
  float *X = (float *)0x100000000ull, *W = (float *)0x200000000ull, *B = (float *)0x300000000ull;
  float *Y = (float *)0x400000000ull, *DX = (float *)0x500000000ull, *GW = (float *)0x600000000ull;
  float *GB = (float *)0x700000000ull, *PL = (float *)0x800000000ull;
  unsigned char *MK = (unsigned char *)0x900000000ull;
  void *WS = (void *)0xa00000000ull;

  static const int shapes[][8] = {
      // H, W, C, kh, kw, G, pad_h, pad_w
      {40, 11, 3, 8, 1, 128, 0, 0}, {40, 21, 1, 40, 4, 128, 0, 0}, {1, 18, 128, 1, 3, 128, 0, 0},
      {8, 9, 256, 3, 3, 32, 1, 1}, {4, 9, 64, 4, 3, 256, 0, 0}, {5, 6, 2, 3, 3, 5, 1, 2},
      {3, 4, 1, 2, 2, 3, 0, 0}, {40, 11, 3, 8, 1, 256, 0, 0}, {8, 9, 256, 3, 3, 256, 1, 1},
      {11, 11, 64, 4, 3, 256, 0, 0}, {7, 8, 16, 3, 3, 128, 1, 1}, {4, 4, 32, 3, 3, 128, 1, 1},
      {6, 7, 9, 3, 3, 64, 1, 1}, {5, 6, 11, 3, 3, 128, 1, 0}, {12, 10, 4, 5, 5, 32, 1, 1},
      {6, 7, 8, 3, 3, 320, 1, 1}, {9, 10, 5, 3, 5, 96, 0, 0}, {7, 7, 4, 5, 5, 64, 2, 2},
      {1, 4, 40, 1, 3, 64, 0, 0}, {7, 6, 4, 3, 3, 32, 0, 0}, {40, 20, 4, 5, 2, 128, 0, 0},
      {20, 13, 8, 3, 1, 32, 0, 0}, {6, 5, 4, 3, 3, 16, 1, 1}, {41, 11, 1, 8, 3, 64, 0, 0},
      {12, 10, 2, 3, 3, 32, 1, 1}, {40, 5, 1, 31, 1, 96, 0, 0}, {35, 16, 1, 4, 1, 32, 0, 0},
      {5, 5, 2, 2, 2, 128, 0, 0}, {8, 40, 1, 8, 3, 64, 0, 0}, {9, 7, 2, 2, 3, 224, 0, 0},
      {9, 5, 1, 2, 2, 64, 0, 0}, {10, 6, 2, 4, 4, 64, 0, 0}, {10, 6, 2, 4, 4, 128, 0, 0},
      {2, 3, 1168, 2, 1, 64, 0, 0}, {3, 4, 10, 3, 3, 10, 1, 1}, {5, 6, 3, 2, 2, 2, 0, 0},
      {9, 9, 2, 2, 2, 130, 0, 0}, {9, 9, 2, 2, 2, 200, 0, 0}, {9, 9, 2, 2, 2, 160, 0, 0},
      {30, 30, 2, 3, 3, 64, 0, 0}, {60, 40, 1, 5, 5, 32, 0, 0}, {24, 24, 3, 3, 3, 96, 1, 1},
      {16, 13, 2, 4, 4, 128, 0, 0}, {40, 11, 3, 8, 1, 64, 0, 0}, {40, 11, 1, 8, 1, 128, 0, 0},
      {14, 9, 64, 7, 5, 36, 3, 2}, {3, 3, 4, 5, 5, 16, 0, 0}, {40, 11, 3, 8, 1, 0, 0, 0},
      {12, 12, 1, 6, 6, 128, 0, 0}, {12, 12, 1, 4, 8, 96, 1, 1}, {20, 20, 5, 2, 3, 128, 0, 0},
      {12, 12, 3, 4, 8, 64, 1, 1}, {12, 12, 3, 4, 8, 128, 1, 1}, {2, 3, 1168, 2, 1, 128, 0, 0},
      // short kernels past the fused backward's map limits (C*H*W > 2048 or P > 512)
      {22, 12, 8, 3, 1, 32, 1, 0}, {33, 16, 4, 2, 2, 64, 0, 0}, {20, 13, 8, 3, 1, 256, 0, 0},
      {20, 13, 8, 3, 1, 160, 0, 0}, {36, 16, 1, 3, 1, 32, 0, 0}, {33, 16, 4, 2, 2, 64, 1, 1},
      {40, 61, 1, 8, 3, 256, 0, 0}, {43, 13, 1, 2, 2, 128, 0, 0},
  };
  std::vector<Job> jobs;
  if (argc == 2) {  // the built-in sweep
    for (auto &s : shapes) {
      Job j{{}, {0, 1, 9, 300, 4096, 9000}};
      memcpy(j.s, s, sizeof j.s);
      jobs.push_back(j);
    }
  } else if (argc == 3 && strcmp(argv[2], "-") == 0) {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
      Job j;
      if (line[strspn(line, " \t\r\n")] == 0) continue;
      if (!parse_job(line, j)) return 2;
      jobs.push_back(j);
    }
  } else {
    for (int a = 2; a < argc; a++) {
      Job j;
      if (!parse_job(argv[a], j)) return 2;
      jobs.push_back(j);
    }
  }
  for (auto &job : jobs) {
    const int *s = job.s;
    const std::vector<int> &rows = job.rows;
    const int H = s[0], Wd = s[1], C = s[2], kh = s[3], kw = s[4], G = s[5], ph_ = s[6], pw_ = s[7];
    const int oh = H + 2 * ph_ - kh + 1, ow = Wd + 2 * pw_ - kw + 1, P = oh * ow, Kd = kh * kw * C;
    for (int R : rows) {
      for (int mis = 0; mis < 2; mis++) {  // mis: odd strides and 4-byte-aligned pointers
        const int xs = H * Wd * C + (mis ? 1 : 0), ys = P * G + (mis ? 3 : 0), ksd = G + (mis ? 1 : 0);
        float *Xp = X + mis, *Wp = W + mis, *Yp = Y + mis, *DXp = DX + mis;
        MatrixDim xd = md(R, H * Wd * C, xs), kd = md(Kd, G, ksd), yd = md(R, P * G, ys);
        MatrixDim gwd = md(Kd, G), dxd = md(R, H * Wd * C, xs), ypl = md(R * P, G);
        printf("shape %d %d %d %d %d %d %d %d R %d mis %d\n", H, Wd, C, kh, kw, G, ph_, pw_, R, mis);
        MatrixDim xd1 = md(R ? R : 1, H * Wd * C, xs), yd1 = md(R ? R : 1, P * G, ys);
        const size_t wf = ws_f(xd1, H, Wd, C, ph_, pw_, kh, kw, G), ww = ws_w(xd1, H, Wd, C, ph_, pw_, kh, kw, G);
        const size_t wd = ws_d(yd1, H, Wd, C, ph_, pw_, kh, kw, G), wb = ws_b(xd1, H, Wd, C, ph_, pw_, kh, kw, G);
        printf(" ws %zu %zu %zu %zu\n", wf, ww, wd, wb);
        for (int wsel = 0; wsel < 2; wsel++) {  // full workspace, none
          void *wsp = wsel ? nullptr : WS;
          const size_t big = wsel ? 0 : ((size_t)1 << 40);
          printf(" conv2d concat -> %d\n", conv2d(Xp, xd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, Yp, yd, 1, wsp, wsel ? 0 : wf, nullptr));
          printf(" conv2d plain -> %d\n", conv2d(Xp, xd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, Yp, ypl, 0, wsp, wsel ? 0 : wf, nullptr));
          printf(" wgrad -> %d\n", wgrad(Xp, xd, H, Wd, C, ph_, pw_, Yp, yd, kh, kw, G, GW, gwd, GB, wsp, wsel ? 0 : ww, nullptr));
          printf(" dgrad -> %d\n", dgrad(Yp, yd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, DXp, dxd, wsp, wsel ? 0 : wd, nullptr));
          printf(" backward -> %d\n", backward(Xp, xd, H, Wd, C, ph_, pw_, Yp, yd, Wp, kd, kh, kw, G, DXp, dxd, GW, gwd, GB, wsp, wsel ? 0 : wb, nullptr));
          printf(" backward nodx -> %d\n", backward(Xp, xd, H, Wd, C, ph_, pw_, Yp, yd, Wp, kd, kh, kw, G, nullptr, dxd, GW, gwd, GB, wsp, big, nullptr));
          if (wsel) continue;
          printf(" relu -> %d\n", relu(Xp, xd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, Yp, yd, nullptr));
          for (int pc : {2, 4, 8, 3}) {
            if (G % pc) continue;
            MatrixDim pd = md(R, P * G / pc);
            printf(" maxpool pc %d -> %d\n", pc, maxpool(Xp, xd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, Yp, yd, PL, pd, MK, P * G / pc, pc, nullptr));
            printf(" maxpool pc %d noY -> %d\n", pc, maxpool(Xp, xd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, nullptr, yd, PL, pd, MK, P * G / pc, pc, nullptr));
            printf(" bpool pc %d -> %d\n", pc, bpool(Xp, xd, H, Wd, C, ph_, pw_, MK, P * G / pc, PL, pd, pc, Wp, kd, kh, kw, G, DXp, dxd, GW, gwd, GB, WS, big, nullptr));
            printf(" bpool pc %d nodx -> %d\n", pc, bpool(Xp, xd, H, Wd, C, ph_, pw_, MK, P * G / pc, PL, pd, pc, Wp, kd, kh, kw, G, nullptr, dxd, GW, gwd, GB, WS, big, nullptr));
            printf(" bpool pc %d nogw -> %d\n", pc, bpool(Xp, xd, H, Wd, C, ph_, pw_, MK, P * G / pc, PL, pd, pc, Wp, kd, kh, kw, G, DXp, dxd, nullptr, gwd, nullptr, WS, big, nullptr));
            for (int ph : {2, 3}) {
              if (oh <= 0 || oh % ph) continue;
              MatrixDim p3 = md(R, P * G / pc / ph);
              printf(" maxpool3d %dx1x%d -> %d\n", ph, pc, maxpool3d(Xp, xd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, Yp, yd, PL, p3, (unsigned short *)MK, P * G / pc / ph, ph, 1, pc, nullptr));
              printf(" bpool3d %dx1x%d -> %d\n", ph, pc, bpool3(Xp, xd, H, Wd, C, ph_, pw_, (unsigned short *)MK, P * G / pc / ph, PL, p3, ph, 1, pc, Wp, kd, kh, kw, G, DXp, dxd, GW, gwd, GB, WS, big, nullptr));
            }
            if (ow > 0 && ow % 2 == 0) {
              MatrixDim p3 = md(R, P * G / pc / 2);
              printf(" maxpool3d 1x2x%d -> %d\n", pc, maxpool3d(Xp, xd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, Yp, yd, PL, p3, (unsigned short *)MK, P * G / pc / 2, 1, 2, pc, nullptr));
            }
          }
        }
        // argument errors: a wrong column count on each matrix
        MatrixDim bad = md(R, H * Wd * C + 1);
        printf(" bad in -> %d %d %d\n", conv2d(Xp, bad, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, B, Yp, yd, 1, WS, wf, nullptr),
               wgrad(Xp, bad, H, Wd, C, ph_, pw_, Yp, yd, kh, kw, G, GW, gwd, GB, WS, ww, nullptr),
               backward(Xp, bad, H, Wd, C, ph_, pw_, Yp, yd, Wp, kd, kh, kw, G, DXp, dxd, GW, gwd, GB, WS, wb, nullptr));
        MatrixDim badk = md(Kd + 1, G);
        printf(" bad kernel -> %d %d %d\n", conv2d(Xp, xd, H, Wd, C, ph_, pw_, Wp, badk, kh, kw, G, B, Yp, yd, 1, WS, wf, nullptr),
               dgrad(Yp, yd, H, Wd, C, ph_, pw_, Wp, badk, kh, kw, G, DXp, dxd, WS, wd, nullptr),
               wgrad(Xp, xd, H, Wd, C, ph_, pw_, Yp, yd, kh, kw, G, GW, badk, GB, WS, ww, nullptr));
        printf(" bad dx / null gw -> %d %d %d\n", dgrad(Yp, yd, H, Wd, C, ph_, pw_, Wp, kd, kh, kw, G, DXp, bad, WS, wd, nullptr),
               backward(Xp, xd, H, Wd, C, ph_, pw_, Yp, yd, Wp, kd, kh, kw, G, DXp, bad, GW, gwd, GB, WS, wb, nullptr),
               backward(Xp, xd, H, Wd, C, ph_, pw_, Yp, yd, Wp, kd, kh, kw, G, DXp, dxd, nullptr, gwd, GB, WS, wb, nullptr));
      }
    }
  }
  return 0;
}
