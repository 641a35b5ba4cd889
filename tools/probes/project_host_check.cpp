// Host check of the projection matcher's query-side arithmetic (pislam_amd/csrc/pislam_project_math.h, shared with the
// kernel), on the CPU only: reads queries, runs steps 1-6 of pislam_match_projection_batch's contract (pjm::frame_ok,
// pjm::project) and prints what the match would start from.  tests/test_match_projection.py compares the words with its
// numpy restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/project_host_check.cpp -o project_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   project_host_check cases.txt        (or the cases on standard input)
// One query per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   nlevels has_normal has_drange qlevel  pose[12] cam[5] xw[3]  normal[3] (if has_normal)  drange[2] (if has_drange)
//   level_scale[nlevels] radius_far[nlevels] radius_near[nlevels]  min_x max_x min_y max_y cos_min cos_near
// (qlevel is -1 in map mode; map mode is has_drange 1.)  One line of output per query:
//   live xc yc pl near r        (a dead query prints 0 0 0 255 0 0)
#include <vector>
#include "hex_words.h"
#include "pislam_project_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int queries = 0;
  for (;;) {
    int nlevels, has_normal, has_drange, qlevel;
    const int got = fscanf(f, "%d %d %d %d", &nlevels, &has_normal, &has_drange, &qlevel);
    if (got == EOF) break;
    if (got != 4 || nlevels < 1 || nlevels > pjm::MAX_LEVELS || (has_drange != 0) == (qlevel >= 0) || qlevel > 255 ||
        (has_normal && !has_drange))
      return fprintf(stderr, "query %d: bad header\n", queries), 2;
    // heap copies of exactly the sizes the procedure may touch: a read past them is an ASan report
    std::vector<float> pose(12), cam(5), xw(3), normal(has_normal ? 3 : 0), drange(has_drange ? 2 : 0), ls((size_t)nlevels);
    float T[12], C[5], par[6];
    pjm::Tables tab{};
    bool ok = true;
    for (auto &v : pose) ok = ok && rd_f32(f, &v);
    for (auto &v : cam) ok = ok && rd_f32(f, &v);
    for (auto &v : xw) ok = ok && rd_f32(f, &v);
    for (auto &v : normal) ok = ok && rd_f32(f, &v);
    for (auto &v : drange) ok = ok && rd_f32(f, &v);
    for (auto &v : ls) ok = ok && rd_f32(f, &v);
    for (int t = 0; ok && t < 2; t++)
      for (int l = 0; ok && l < nlevels; l++) {
        long long r;
        ok = fscanf(f, "%lld", &r) == 1 && r >= 0 && r <= pjm::MAX_RADIUS;
        (t ? tab.radius_near : tab.radius_far)[l] = (int32_t)r;
      }
    for (auto &v : par) ok = ok && rd_f32(f, &v);
    if (!ok) return fprintf(stderr, "query %d: truncated\n", queries), 2;
    for (int l = 0; l < nlevels; l++) tab.level_scale[l] = ls[(size_t)l];
    tab.nlevels = nlevels;
    for (int i = 0; i < 12; i++) T[i] = pose[(size_t)i];
    for (int i = 0; i < 5; i++) C[i] = cam[(size_t)i];
    const pjm::Params prm{par[0], par[1], par[2], par[3], par[4], par[5], 0, 0, 0};
    pjm::Query q{false, false, 0, 0, pjm::DEAD_LEVEL, 0};
    if (pjm::frame_ok(pose.data(), cam.data()))
      q = pjm::project(T, C, xw.data(), has_normal ? normal.data() : nullptr, has_drange ? drange.data() : nullptr, qlevel,
                       tab, prm);
    printf("%d %" PRId32 " %" PRId32 " %" PRId32 " %d %" PRId32 "\n", q.live ? 1 : 0, q.xc, q.yc, q.pl, q.near ? 1 : 0, q.r);
    queries++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
