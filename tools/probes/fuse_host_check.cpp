// Host check of the fuse matcher's per-candidate arithmetic (pislam_amd/csrc/pislam_project_math.h, shared with the
// kernel), on the CPU only: reads a query and one candidate keypoint per line, runs steps 1-6 of
// pislam_match_fuse_batch's contract (pjm::frame_ok, pjm::project with the pixel handed out) and the reprojection test
// of step 7 (pjm::fuse_ok), and prints what the match would start from plus the candidate's verdict.
// tests/test_match_fuse.py compares the words with its numpy restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/fuse_host_check.cpp -o fuse_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   fuse_host_check cases.txt        (or the cases on standard input)
// One query and candidate per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal
// integers.  The first part is project_host_check's line:
//   nlevels has_normal has_drange qlevel  pose[12] cam[5] xw[3]  normal[3] (if has_normal)  drange[2] (if has_drange)
//   level_scale[nlevels] radius_far[nlevels] radius_near[nlevels]  min_x max_x min_y max_y cos_min cos_near
// then the candidate:
//   u_q8 v_q8 ur_q8 (INT32_MIN: monocular)  inv_sigma2 (of the candidate's level)  chi2_mono chi2_stereo
// One line of output per query:
//   live xc yc pl near r ok        (a dead query prints 0 0 0 255 0 0 0; ok: the candidate passes the test)
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
    float T[12], C[5], par[6], fus[3];
    long long obs[3];
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
    for (auto &v : obs) ok = ok && fscanf(f, "%lld", &v) == 1 && v >= INT32_MIN && v <= INT32_MAX;
    for (auto &v : fus) ok = ok && rd_f32(f, &v);
    if (!ok) return fprintf(stderr, "query %d: truncated\n", queries), 2;
    for (int l = 0; l < nlevels; l++) tab.level_scale[l] = ls[(size_t)l];
    tab.nlevels = nlevels;
    for (int i = 0; i < 12; i++) T[i] = pose[(size_t)i];
    for (int i = 0; i < 5; i++) C[i] = cam[(size_t)i];
    const pjm::Params prm{par[0], par[1], par[2], par[3], par[4], par[5], 0, 0, 0};
    pjm::Query q{false, false, 0, 0, pjm::DEAD_LEVEL, 0};
    pjm::Pixel px{0.0f, 0.0f, 0.0f};
    if (pjm::frame_ok(pose.data(), cam.data()))
      q = pjm::project(T, C, xw.data(), has_normal ? normal.data() : nullptr, has_drange ? drange.data() : nullptr, qlevel,
                       tab, prm, &px);
    const bool pass = q.live && pjm::fuse_ok(px, (int32_t)obs[0], (int32_t)obs[1], (int32_t)obs[2], fus[0], fus[1], fus[2]);
    printf("%d %" PRId32 " %" PRId32 " %" PRId32 " %d %" PRId32 " %d\n", q.live ? 1 : 0, q.xc, q.yc, q.pl, q.near ? 1 : 0, q.r,
           pass ? 1 : 0);
    queries++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
