// Host check of the new-map-point arithmetic (pislam_amd/csrc/pislam_mappoint_math.h, shared with the kernel), on the
// CPU only: reads slots, runs pislam_triangulate_batch's contract for each (pmp::pair_setup, pmp::slot) and prints every
// output word.  tests/test_triangulate.py compares the words with its numpy restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/mappoint_host_check.cpp -o mappoint_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   mappoint_host_check cases.txt        (or the cases on standard input)
// One slot per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   nlevels level1 level2  obs1[3] obs2[3]  pose1[12] pose2[12] cam1[5] cam2[5]
//   level_scale[nlevels] level_sigma2[nlevels]  cos_min_parallax chi2_mono chi2_stereo ratio_factor
// One line of output per slot:
//   status mode  xw[3] normal[3] drange[2]        (mode: 0 none, 1 triangulated, 2 / 3 unprojected from side 1 / 2)
#include <vector>
#include "hex_words.h"
#include "pislam_mappoint_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int slots = 0;
  for (;;) {
    int nlevels, l1, l2;
    const int got = fscanf(f, "%d %d %d", &nlevels, &l1, &l2);
    if (got == EOF) break;
    if (got != 3 || nlevels < 1 || nlevels > pmp::MAX_LEVELS || l1 < 0 || l1 > 255 || l2 < 0 || l2 > 255)
      return fprintf(stderr, "slot %d: bad header\n", slots), 2;
    // heap copies of exactly the sizes the procedure may touch: a read past them is an ASan report
    std::vector<int32_t> obs1(3), obs2(3);
    std::vector<float> pose1(12), pose2(12), cam1(5), cam2(5), ls((size_t)nlevels), sg((size_t)nlevels);
    float par[4];
    bool ok = true;
    for (auto *o : {&obs1, &obs2})
      for (auto &v : *o) {
        long long q;
        ok = ok && fscanf(f, "%lld", &q) == 1 && q >= INT32_MIN && q <= INT32_MAX;
        v = (int32_t)q;
      }
    for (auto *a : {&pose1, &pose2, &cam1, &cam2, &ls, &sg})
      for (auto &v : *a) ok = ok && rd_f32(f, &v);
    for (auto &v : par) ok = ok && rd_f32(f, &v);
    if (!ok) return fprintf(stderr, "slot %d: truncated\n", slots), 2;
    pmp::Tables tab{};
    tab.nlevels = nlevels;
    for (int l = 0; l < nlevels; l++) tab.level_scale[l] = ls[(size_t)l], tab.level_sigma2[l] = sg[(size_t)l];
    const pmp::Params prm{par[0], par[1], par[2], par[3]};
    pmp::Pair P;
    pmp::Slot s{pmp::PAIR, pmp::NONE, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f}};
    if (pmp::pair_setup(pose1.data(), pose2.data(), cam1.data(), cam2.data(), &P))
      s = pmp::slot(P, obs1.data(), obs2.data(), l1, l2, tab, prm);
    printf("%d %d", (int)s.status, (int)s.mode);
    for (float v : s.xw) pr_f32(v);
    for (float v : s.normal) pr_f32(v);
    for (float v : s.drange) pr_f32(v);
    printf("\n");
    slots++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
