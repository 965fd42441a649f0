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
// routes of single shapes this way).  An argument or line that starts with a
// letter is a case of one pooled entry point instead (scripts/README.md has
// the syntax; tests/test_conv_pool_routes.py pins tests/conv_pool_cases.py's
// table this way):
//   ENTRY H,W,C,kh,kw,G,pad_h,pad_w,rows PHxPWxPC OUTS [OPERAND=stride:lead ...]
// and prints "case <k> <entry>", its launches and " rc <return code>" (the
// statistics entry " rc <return code> produced <0 | 1>").  Two builds dispatch
// alike when their logs are equal after scripts/conv_launch_names.py has
// replaced the handle offsets by symbol names (profiles/conv_dispatch.md):
//   g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       scripts/conv_launch_log.cc -o conv_launch_log -rdynamic -ldl
//   ./conv_launch_log kaldi-cnn_amd/libkcnn.so > new.raw
//   ./conv_launch_log kaldi-cnn_amd/libkcnn.so 20,13,8,3,1,32,0,0 40,61,1,8,3,256,0,0,5
//   python scripts/conv_launch_names.py kaldi-cnn_amd/libkcnn.so new.raw > new.txt
#include <string.h>

#include <string>
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

// ---- cases of the pooled entry points -------------------------------------------------------
// PoolStatsOut of src/cnslmat/pool-stats.h (the logger builds against include/ alone)
struct StatsOut {
  uint32_t *rowmax, *colmax, *partials;
  size_t partial_words;
  int produced;
};
typedef int (*maxpool_stats_fn)(const float *, MatrixDim, int, int, int, int, int, const float *,
                                MatrixDim, int, int, int, const float *, float *, MatrixDim,
                                float *, MatrixDim, unsigned char *, int, int, kcnn_stream_t,
                                StatsOut *);
typedef size_t (*stats_words_fn)(int, int, int, int, int, int, int, int);

// an operand's row stride (-1: its columns) and lead, in its own elements
struct Lay {
  int stride = -1, lead = 0;
};

static const char *const kOperands[] = {"x", "w", "y", "p", "m", "dx", "gw"};
enum { OP_X, OP_W, OP_Y, OP_P, OP_M, OP_DX, OP_GW, OP_N };

static int g_case = 0;

// One case line; false (with a message) when it does not parse.
static bool run_case(const char *txt) {
  std::vector<std::string> tok;
  for (const char *p = txt; *p;) {
    p += strspn(p, " \t\r\n");
    const size_t n = strcspn(p, " \t\r\n");
    if (n) tok.emplace_back(p, n);
    p += n;
  }
  int s[9], ph, pw, pc;
  if (tok.size() < 4 ||
      sscanf(tok[1].c_str(), "%d,%d,%d,%d,%d,%d,%d,%d,%d", s, s + 1, s + 2, s + 3, s + 4, s + 5,
             s + 6, s + 7, s + 8) != 9 ||
      sscanf(tok[2].c_str(), "%dx%dx%d", &ph, &pw, &pc) != 3) {
    fprintf(stderr, "bad case: %s\n", txt);
    return false;
  }
  const std::string &entry = tok[0], &outs = tok[3];
  const bool fwd = entry == "maxpool" || entry == "maxpool_stats" || entry == "maxpool_stats0" ||
                   entry == "maxpool3d";
  const bool bwd = entry == "bpool" || entry == "bpool3d" || entry == "backward" ||
                   entry == "dgrad";
  if (!(fwd || bwd) || !(fwd ? outs == "Y" || outs == "noY"
                             : outs == "both" || outs == "nodx" || outs == "nogw")) {
    fprintf(stderr, "bad case: %s\n", txt);
    return false;
  }
  Lay lay[OP_N];
  for (size_t t = 4; t < tok.size(); t++) {
    char name[8];
    int st, ld, k = 0;
    if (sscanf(tok[t].c_str(), "%7[a-z]=%d:%d", name, &st, &ld) != 3) k = OP_N;
    while (k < OP_N && strcmp(name, kOperands[k])) k++;
    if (k == OP_N) {
      fprintf(stderr, "bad operand %s: %s\n", tok[t].c_str(), txt);
      return false;
    }
    lay[k].stride = st;
    lay[k].lead = ld;
  }
  const int H = s[0], Wd = s[1], C = s[2], kh = s[3], kw = s[4], G = s[5], pad_h = s[6],
            pad_w = s[7], R = s[8];
  const int oh = H + 2 * pad_h - kh + 1, ow = Wd + 2 * pad_w - kw + 1, P = oh * ow;
  const int Kd = kh * kw * C, win = ph * pw * pc;
  const int pcols = win > 0 ? (int)((int64_t)P * G / win) : 0;
  auto dim = [&](int k, int rows, int cols) {
    return MatrixDim{rows, cols, lay[k].stride < 0 ? cols : lay[k].stride};
  };
  // each operand in its own 4 GiB of fake address space, 4096-byte aligned
  auto at = [&](int k, size_t elem) {
    return (char *)(0x100000000ull * (uintptr_t)(k + 1)) + (int64_t)lay[k].lead * (int64_t)elem;
  };
  float *X = (float *)at(OP_X, 4), *W = (float *)at(OP_W, 4), *Y = (float *)at(OP_Y, 4);
  float *PL = (float *)at(OP_P, 4), *DX = (float *)at(OP_DX, 4), *GW = (float *)at(OP_GW, 4);
  const bool m16 = entry == "maxpool3d" || entry == "bpool3d";
  unsigned char *MK = (unsigned char *)at(OP_M, m16 ? 2 : 1);
  float *B = (float *)0x900000000ull, *GB = (float *)0x980000000ull;
  void *WS = (void *)0xa00000000ull;
  const size_t big = (size_t)1 << 40;
  const MatrixDim xd = dim(OP_X, R, H * Wd * C), kd = dim(OP_W, Kd, G), yd = dim(OP_Y, R, P * G);
  const MatrixDim pd = dim(OP_P, R, pcols), dxd = dim(OP_DX, R, H * Wd * C);
  const MatrixDim gwd = dim(OP_GW, Kd, G);
  const int ms = lay[OP_M].stride < 0 ? pcols : lay[OP_M].stride;
  printf("case %d %s\n", g_case++, entry.c_str());
  int rc;
  if (fwd) {
    float *Yp = outs == "Y" ? Y : nullptr;
    if (entry == "maxpool") {
      auto f = sym<decltype(&hipF_conv2d_maxpool)>("hipF_conv2d_maxpool");
      rc = f(X, xd, H, Wd, C, pad_h, pad_w, W, kd, kh, kw, G, B, Yp, yd, PL, pd, MK, ms, pc,
             nullptr);
    } else if (entry == "maxpool3d") {
      auto f = sym<decltype(&hipF_conv2d_maxpool3d)>("hipF_conv2d_maxpool3d");
      rc = f(X, xd, H, Wd, C, pad_h, pad_w, W, kd, kh, kw, G, B, Yp, yd, PL, pd,
             (unsigned short *)MK, ms, ph, pw, pc, nullptr);
    } else {
      auto f = sym<maxpool_stats_fn>("kcnn_conv2d_maxpool_stats");
      auto words = sym<stats_words_fn>("kcnn_conv2d_maxpool_stats_words");
      StatsOut st{(uint32_t *)0xb00000000ull, (uint32_t *)0xb80000000ull, nullptr, 0, 0};
      if (entry == "maxpool_stats") {
        st.partials = (uint32_t *)0xc00000000ull;
        st.partial_words = words(R, H, Wd, C, kh, kw, G, pc);
      }
      rc = f(X, xd, H, Wd, C, pad_h, pad_w, W, kd, kh, kw, G, B, Yp, yd, PL, pd, MK, ms, pc,
             nullptr, &st);
      printf(" rc %d produced %d\n", rc, st.produced);
      return true;
    }
  } else {
    float *DXp = outs == "nodx" ? nullptr : DX, *GWp = outs == "nogw" ? nullptr : GW;
    float *GBp = outs == "nogw" ? nullptr : GB;
    if (entry == "bpool") {
      auto f = sym<decltype(&hipF_conv2d_backward_pooled)>("hipF_conv2d_backward_pooled");
      rc = f(X, xd, H, Wd, C, pad_h, pad_w, MK, ms, PL, pd, pc, W, kd, kh, kw, G, DXp, dxd, GWp,
             gwd, GBp, WS, big, nullptr);
    } else if (entry == "bpool3d") {
      auto f = sym<decltype(&hipF_conv2d_backward_pooled3d)>("hipF_conv2d_backward_pooled3d");
      rc = f(X, xd, H, Wd, C, pad_h, pad_w, (const unsigned short *)MK, ms, PL, pd, ph, pw, pc, W,
             kd, kh, kw, G, DXp, dxd, GWp, gwd, GBp, WS, big, nullptr);
    } else if (entry == "backward") {  // the unpooled backward on the same operands (dY in Y's place)
      auto f = sym<decltype(&hipF_conv2d_backward)>("hipF_conv2d_backward");
      rc = f(X, xd, H, Wd, C, pad_h, pad_w, Y, yd, W, kd, kh, kw, G, DXp, dxd, GWp, gwd, GBp, WS,
             big, nullptr);
    } else {  // and the data gradient alone (OUTS nogw)
      auto f = sym<decltype(&hipF_conv2d_dgrad)>("hipF_conv2d_dgrad");
      rc = f(Y, yd, H, Wd, C, pad_h, pad_w, W, kd, kh, kw, G, DX, dxd, WS, big, nullptr);
    }
  }
  printf(" rc %d\n", rc);
  return true;
}

static bool is_case(const char *txt) {
  const char c = txt[strspn(txt, " \t")];
  return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
}

int main(int argc, char **argv) {
  setvbuf(stdout, nullptr, _IONBF, 0);
  if (argc < 2) {
    fprintf(stderr, "usage: %s libkcnn.so [H,W,C,kh,kw,G,pad_h,pad_w[,rows] | 'CASE' ... | -]\n",
            argv[0]);
    return 2;
  }
  open_lib(argv[1]);
  // the arguments, or the lines of standard input: all cases or all shapes
  std::vector<std::string> items;
  if (argc == 3 && strcmp(argv[2], "-") == 0) {
    char line[512];
    while (fgets(line, sizeof line, stdin))
      if (line[strspn(line, " \t\r\n")] != 0) items.emplace_back(line);
  } else {
    for (int a = 2; a < argc; a++) items.emplace_back(argv[a]);
  }
  if (!items.empty() && is_case(items[0].c_str())) {
    for (auto &it : items)
      if (!is_case(it.c_str()) || !run_case(it.c_str())) return 2;
    return 0;
  }
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
  } else {
    for (auto &it : items) {
      Job j;
      if (!parse_job(it.c_str(), j)) return 2;
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
