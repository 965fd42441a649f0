// scripts/time_plan_config.h -- what the stand-alone check programs of the time
// plan (time_plan_check.cc, time_plan_height_check.cc, time_schedule_check.cc)
// share: a network config parsed line by line into the plan's TimeComps, as
// NnetStack::TimeSharedPlan fills them from the components, and the counting
// `expect`.  Host only; one program includes it once.
#ifndef KCNN_SCRIPTS_TIME_PLAN_CONFIG_H_
#define KCNN_SCRIPTS_TIME_PLAN_CONFIG_H_

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "capi/time-plan.h"

namespace {

int failures = 0;
long checks = 0;

void expect(bool ok, const char *what, long a = 0, long b = 0) {
  checks++;
  if (ok) return;
  if (failures < 20) printf("WRONG: %s (%ld, %ld)\n", what, a, b);
  failures++;
}

// ---- a config line -> TimeComp ------------------------------------------------
kcnn::TimeComp parse_line(const std::string &line) {
  using kcnn::TimeComp;
  std::istringstream is(line);
  std::string type, tok;
  is >> type;
  std::map<std::string, std::string> kv;
  while (is >> tok) {
    const size_t eq = tok.find('=');
    if (eq != std::string::npos) kv[tok.substr(0, eq)] = tok.substr(eq + 1);
  }
  auto num = [&](const char *k, int def = 0) {
    return kv.count(k) ? atoi(kv[k].c_str()) : def;
  };
  TimeComp c;
  if (type == "SpliceComponent") {
    c.kind = TimeComp::kSplice;
    c.input_dim = num("input-dim");
    c.left = num("left-context");
    c.right = num("right-context");
    c.contiguous = !kv.count("context");
    c.const_dim = num("const-component-dim");
    c.output_dim = c.input_dim * (c.left + c.right + 1);
  } else if (type == "ConvolutionComponent") {
    c.kind = TimeComp::kConv;
    c.in_height = num("in-height");
    c.in_width = num("in-width");
    c.in_channel = num("in-channel");
    c.kernel_height = num("kernel-height");
    c.kernel_width = num("kernel-width");
    c.stride = num("stride", 1);
    c.pad_height = num("in-pad-height");
    c.pad_width = num("in-pad-width");
    c.group = num("group");
    c.out_height = num("out-height");
    c.out_width = num("out-width");
    c.input_dim = c.in_height * c.in_width * c.in_channel;
    c.output_dim = c.out_height * c.out_width * c.group;
  } else if (type == "MaxpoolComponent") {
    c.kind = TimeComp::kPool;
    c.in_height = num("in-height");
    c.in_width = num("in-width");
    c.in_channel = num("in-channel");
    c.pool_height = num("pool-height-dim");
    c.pool_width = num("pool-width-dim");
    c.pool_channel = num("pool-channel-dim");
    c.input_dim = c.in_height * c.in_width * c.in_channel;
    c.output_dim = c.input_dim / (c.pool_height * c.pool_width * c.pool_channel);
  } else if (type == "RectifiedLinearComponent") {
    c.kind = TimeComp::kRelu;
    c.input_dim = c.output_dim = num("dim");
  } else {
    c.input_dim = kv.count("dim") ? num("dim") : num("input-dim");
    c.output_dim = kv.count("dim") ? num("dim") : num("output-dim");
  }
  return c;
}

std::vector<kcnn::TimeComp> parse_config(const std::string &text) {
  std::vector<kcnn::TimeComp> out;
  std::istringstream is(text);
  std::string line;
  while (std::getline(is, line)) {
    const size_t b = line.find_first_not_of(" \t\r");
    if (b == std::string::npos || line[b] == '#') continue;
    out.push_back(parse_line(line.substr(b)));
  }
  return out;
}

}  // namespace

#endif  // KCNN_SCRIPTS_TIME_PLAN_CONFIG_H_
