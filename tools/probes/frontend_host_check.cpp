// Host check of the front end's planner (pislam_amd/csrc/pislam_frontend_plan.h: fp::set_option, fp::check_params,
// fp::plan_frontend and the two invariant checkers), on the CPU only.  Every case of a text file goes through them the way
// pislam_debug_build_plan does; a plan that violates an invariant the kernels rely on makes the program exit non-zero.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pislam_amd/csrc tools/probes/frontend_host_check.cpp -o tools/probes/_bin/frontend_host_check
//   tools/probes/_bin/frontend_host_check tests/golden/frontend_plan_cases.txt       (the fixed cases)
//   python tests/plan_fuzz.py lines 20000 100000 > cases.txt && tools/probes/_bin/frontend_host_check cases.txt   (seeded ones)
// A case is one line (tests/plan_fuzz.py case_line writes them): name, the ten pislam_frontend_params fields, batch, CUs,
// lanes, the options as key=value,key=value (- for none), then width height row0 col0 of every level.
// --dump prints one line per case, `name: <fp::plan_digest>` (tests/test_frontend_plan_golden.py holds each line to its recorded hash).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "pislam_frontend_plan.h"

struct Case {
  std::string name, options;
  pislam_frontend_params par;
  int batch = 0, cus = 0, lanes = 0;
  std::vector<pislam_level> levels;
};

static bool parse_case(const std::string &line, Case *c) {
  std::istringstream in(line);
  pislam_frontend_params &p = c->par;
  in >> c->name >> p.vstep >> p.rows >> p.nlevels >> p.border >> p.fast_threshold >> p.harris_threshold >> p.log_bucket_size >>
      p.bucket_limit >> p.words >> p.max_keypoints >> c->batch >> c->cus >> c->lanes >> c->options;
  if (!in) return false;
  pislam_level l;
  while (in >> l.width >> l.height >> l.row0 >> l.col0) c->levels.push_back(l);
  return in.eof() && (int)c->levels.size() == p.nlevels;   // (the planner reads nlevels entries of the table)
}

// The options string, as pislam_debug_build_plan reads it: the first refusal, or nullptr.
static const char *set_options(const std::string &options, fp::Options *o) {
  if (options == "-") return nullptr;
  std::istringstream in(options);
  for (std::string kv; std::getline(in, kv, ',');) {
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return "options: key=value[,key=value...]";
    const char *refusal = nullptr;
    if (!fp::set_option(*o, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1), &refusal)) return "unknown option";
    if (refusal) return refusal;
  }
  return nullptr;
}

int main(int argc, char **argv) {
  bool dump = false;
  const char *path = nullptr;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--dump")) dump = true;
    else path = argv[i];
  }
  std::ifstream file(path ? path : "");
  if (!file) {
    fprintf(stderr, "usage: frontend_host_check [--dump] <cases file>\n");
    return 2;
  }
  int cases = 0, planned = 0, staged = 0, refused = 0, violations = 0;
  for (std::string line; std::getline(file, line);) {
    if (line.empty() || line[0] == '#') continue;
    Case c;
    if (!parse_case(line, &c)) {
      fprintf(stderr, "malformed case: %.60s\n", line.c_str());
      return 2;
    }
    cases++;
    fp::Options o;
    o.num_cus = c.cus > 0 ? c.cus : 256;
    o.lanes_in_flight = c.lanes > 0 ? c.lanes : 1;
    fp::FrontendPlan P;
    const char *refusal = set_options(c.options, &o);
    if (!refusal) refusal = fp::check_params(&c.par, c.levels.data(), c.batch);
    const char *violated = nullptr;
    if (!refusal) {
      refusal = fp::plan_frontend(o, &c.par, c.levels.data(), c.batch, &P);
      if (P.fused) violated = fp::strip_plan_violation(P, &c.par);
      if (P.fused && !violated && !refusal && P.sel) violated = fp::select_plan_violation(P, &c.par);
    }
    if (violated) {
      fprintf(stderr, "%s: plan invariant violated: %s\n", c.name.c_str(), violated);
      violations++;
    }
    if (refusal) refused++;
    else if (P.fused) planned++;
    else staged++;
    if (dump) printf("%s: %s\n", c.name.c_str(), fp::plan_digest(refusal, P).data());
  }
  if (!dump)
    printf("%d cases: %d planned, %d left to the staged pipeline, %d refused, %d violations\n", cases, planned, staged, refused, violations);
  return violations ? 1 : 0;
}
