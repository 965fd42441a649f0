// scripts/nnet2_launch_log.cc -- what the kn_* launchers of src/nnet2/ would
// launch, without a GPU (conv_launch_log.cc's counterpart; the interposed
// hipLaunchKernel and friends are launch_log.h's).  Loads the libkcnn.so given
// as argv[1] and reads cases from standard input, one per line, each a list of
// integers separated by blanks: the launcher's number, then its arguments.
// An operand is four integers, "rows cols stride lead": its MatrixDim and the
// floats between a 4096-byte aligned address and its base (lead -1: a NULL
// pointer).  Operands are fake device pointers, never dereferenced.
//
//    0 kn_relu_prop             in out
//    1 kn_relu_backprop         out_value out_deriv in_deriv stats
//    2 kn_splice_prop           in out GEOM
//    3 kn_splice_backprop       out_deriv in_deriv GEOM
//    4 kn_dvec_update           n x_null
//    5 kn_softmax_prop          in out
//    6 kn_softmax_backprop      out_value out_deriv in_deriv stats
//    7 kn_comp_objf_and_deriv   probs deriv num
//    8 kn_softmax_xent_backprop out_value in_deriv stats
//    9 kn_objf_accuracy         probs
//   10 kn_softmax_objf_accuracy logits
//   11 kn_loglikes              probs out
//   12 kn_softmax_loglikes      logits out
//   13 kn_normalize_prop        in out
//   14 kn_normalize_backprop    in_value out_deriv in_deriv
//   15 kn_timemap_epilogue      in pooled relu rows pool_width pool_channel delta
//   16 kn_timemap_gather        map out num_utts ext positions dilation
//
// stats: 0 none (value_sum NULL), 1 with the workspace, 2 value_sum without a
// workspace.  GEOM: num_chunks in_cs out_cs in_first out_first dim const_dim
// num_splice table, then num_splice context offsets, then with table = 1 the
// num_splice * out_cs entries of in_index.
//
// Prints per case "case <k>", its launches and " rc <return code>":
//   g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       -Ikaldi-cnn_amd/src/nnet2 scripts/nnet2_launch_log.cc -o nnet2_launch_log -rdynamic -ldl
//   ./nnet2_launch_log kaldi-cnn_amd/libkcnn.so < cases.txt > new.raw
//   python scripts/conv_launch_names.py --short kaldi-cnn_amd/libkcnn.so new.raw
// (tests/test_nnet2_routes.py pins tests/nnet2_kernel_cases.py's table this way).
#include <string.h>

#include <algorithm>
#include <vector>

#include "nnet-kernels.h"
#include "launch_log.h"

namespace {

struct Args {
  std::vector<long> v;
  size_t at = 0;
  bool bad = false;
  int next() {
    if (at >= v.size()) { bad = true; return 0; }
    return (int)v[at++];
  }
};

struct Op {
  float *p;
  MatrixDim d;
};

// the k-th operand of a case: its own 4 GiB of fake address space
Op operand(Args &a, int k) {
  Op o;
  o.d.rows = a.next();
  o.d.cols = a.next();
  o.d.stride = a.next();
  const int lead = a.next();
  o.p = lead < 0 ? nullptr : (float *)(0x100000000ull * (uintptr_t)(k + 1)) + lead;
  return o;
}

kn_splice_geom splice_geom(Args &a) {
  kn_splice_geom g;
  memset(&g, 0, sizeof g);
  g.num_chunks = a.next(); g.in_cs = a.next(); g.out_cs = a.next();
  g.in_first = a.next(); g.out_first = a.next();
  g.dim = a.next(); g.const_dim = a.next(); g.num_splice = a.next();
  g.table = a.next();
  const int nc = std::max(0, std::min(g.num_splice, KN_SPLICE_MAX_CONTEXT));
  for (int c = 0; c < nc; c++) g.context[c] = a.next();
  if (g.table) {
    const long nt = std::max(0L, std::min((long)g.num_splice * g.out_cs, (long)KN_SPLICE_MAX_TAB));
    for (long e = 0; e < nt; e++) g.in_index[e] = (short)a.next();
  }
  return g;
}

}  // namespace

int main(int argc, char **argv) {
  setvbuf(stdout, nullptr, _IONBF, 0);
  if (argc != 2) {
    fprintf(stderr, "usage: %s libkcnn.so < cases\n", argv[0]);
    return 2;
  }
  open_lib(argv[1]);
  auto relu_prop = sym<decltype(&kn_relu_prop)>("kn_relu_prop");
  auto relu_backprop = sym<decltype(&kn_relu_backprop)>("kn_relu_backprop");
  auto splice_prop = sym<decltype(&kn_splice_prop)>("kn_splice_prop");
  auto splice_backprop = sym<decltype(&kn_splice_backprop)>("kn_splice_backprop");
  auto dvec_update = sym<decltype(&kn_dvec_update)>("kn_dvec_update");
  auto softmax_prop = sym<decltype(&kn_softmax_prop)>("kn_softmax_prop");
  auto softmax_backprop = sym<decltype(&kn_softmax_backprop)>("kn_softmax_backprop");
  auto comp_objf = sym<decltype(&kn_comp_objf_and_deriv)>("kn_comp_objf_and_deriv");
  auto xent = sym<decltype(&kn_softmax_xent_backprop)>("kn_softmax_xent_backprop");
  auto objf_acc = sym<decltype(&kn_objf_accuracy)>("kn_objf_accuracy");
  auto sm_objf_acc = sym<decltype(&kn_softmax_objf_accuracy)>("kn_softmax_objf_accuracy");
  auto loglikes = sym<decltype(&kn_loglikes)>("kn_loglikes");
  auto sm_loglikes = sym<decltype(&kn_softmax_loglikes)>("kn_softmax_loglikes");
  auto norm_prop = sym<decltype(&kn_normalize_prop)>("kn_normalize_prop");
  auto norm_backprop = sym<decltype(&kn_normalize_backprop)>("kn_normalize_backprop");
  auto epilogue = sym<decltype(&kn_timemap_epilogue)>("kn_timemap_epilogue");
  auto gather = sym<decltype(&kn_timemap_gather)>("kn_timemap_gather");

  // what is no matrix: workspaces (16-byte aligned), totals, labels, tables
  void *WS = (void *)0xa00000000ull, *WS2 = (void *)0xa80000000ull;
  double *SUM = (double *)0xb00000000ull, *SUM2 = (double *)0xb80000000ull;
  double *TOT = (double *)0xc00000000ull;
  int *IA = (int *)0xd00000000ull, *IB = (int *)0xd40000000ull;
  float *FW = (float *)0xd80000000ull;

  char line[16384];
  int k = 0;
  while (fgets(line, sizeof line, stdin)) {
    Args a;
    for (char *p = line, *e;; p = e) {
      const long x = strtol(p, &e, 10);
      if (e == p) break;
      a.v.push_back(x);
    }
    if (a.v.empty()) continue;
    printf("case %d\n", k++);
    const int which = a.next();
    int rc = -1;
    auto stats = [&](double **sum, void **ws) {
      const int s = a.next();
      *sum = s ? SUM : nullptr;
      *ws = s == 1 ? WS : nullptr;
    };
    switch (which) {
      case 0: {
        Op in = operand(a, 0), out = operand(a, 1);
        if (!a.bad) rc = relu_prop(in.p, in.d, out.p, out.d, nullptr);
        break;
      }
      case 1: {
        Op ov = operand(a, 0), od = operand(a, 1), id = operand(a, 2);
        double *sum; void *ws;
        stats(&sum, &ws);
        if (!a.bad)
          rc = relu_backprop(ov.p, ov.d, od.p, od.d, id.p, id.d, sum, sum ? SUM2 : nullptr, ws,
                             nullptr);
        break;
      }
      case 2: case 3: {
        Op x = operand(a, 0), y = operand(a, 1);
        const kn_splice_geom g = splice_geom(a);
        if (!a.bad)
          rc = which == 2 ? splice_prop(x.p, x.d, y.p, y.d, g, nullptr)
                          : splice_backprop(x.p, x.d, y.p, y.d, g, nullptr);
        break;
      }
      case 4: {
        const int n = a.next(), x_null = a.next();
        if (!a.bad) rc = dvec_update(SUM, x_null ? nullptr : SUM2, 0.5, 2.0, n, nullptr);
        break;
      }
      case 5: case 11: case 12: case 13: {
        Op in = operand(a, 0), out = operand(a, 1);
        if (a.bad) break;
        if (which == 5) rc = softmax_prop(in.p, in.d, out.p, out.d, nullptr);
        else if (which == 11) rc = loglikes(in.p, in.d, out.p, out.d, SUM, nullptr);
        else if (which == 12) rc = sm_loglikes(in.p, in.d, out.p, out.d, SUM, nullptr);
        else rc = norm_prop(in.p, in.d, out.p, out.d, nullptr);
        break;
      }
      case 6: {
        Op ov = operand(a, 0), od = operand(a, 1), id = operand(a, 2);
        double *sum; void *ws;
        stats(&sum, &ws);
        if (!a.bad) rc = softmax_backprop(ov.p, ov.d, od.p, od.d, id.p, id.d, sum, ws, nullptr);
        break;
      }
      case 7: {
        Op p = operand(a, 0), d = operand(a, 1);
        const int num = a.next();
        if (!a.bad) rc = comp_objf(IA, IB, FW, num, p.p, p.d, d.p, d.d, TOT, WS2, nullptr);
        break;
      }
      case 8: {
        Op ov = operand(a, 0), id = operand(a, 1);
        double *sum; void *ws;
        stats(&sum, &ws);
        if (!a.bad) rc = xent(ov.p, ov.d, id.p, id.d, IA, IB, FW, sum, ws, TOT, WS2, nullptr);
        break;
      }
      case 9: case 10: {
        Op x = operand(a, 0);
        if (!a.bad)
          rc = (which == 9 ? objf_acc : sm_objf_acc)(x.p, x.d, IA, IB, FW, TOT, WS2, nullptr);
        break;
      }
      case 14: {
        Op iv = operand(a, 0), od = operand(a, 1), id = operand(a, 2);
        if (!a.bad) rc = norm_backprop(iv.p, iv.d, od.p, od.d, id.p, id.d, nullptr);
        break;
      }
      case 15: {
        Op in = operand(a, 0), p = operand(a, 1), r = operand(a, 2);
        const int rows = a.next(), pw = a.next(), pc = a.next(), delta = a.next();
        if (!a.bad) rc = epilogue(in.p, in.d, p.p, p.d, r.p, r.d, rows, pw, pc, delta, nullptr);
        break;
      }
      case 16: {
        Op map = operand(a, 0), out = operand(a, 1);
        const int num_utts = a.next(), ext = a.next(), n = a.next(), dil = a.next();
        if (!a.bad) rc = gather(map.p, map.d, out.p, out.d, IA, num_utts, ext, n, dil, nullptr);
        break;
      }
      default:
        a.bad = true;
    }
    if (a.bad || a.at != a.v.size()) {
      fprintf(stderr, "bad case %d: %s", k - 1, line);
      return 2;
    }
    printf(" rc %d\n", rc);
  }
  return 0;
}
