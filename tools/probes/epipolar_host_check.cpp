// Host check of the epipolar matcher's geometric test (pislam_amd/csrc/pislam_epipolar_math.h, shared with the kernels),
// on the CPU only: reads (query, train) keypoint pairs, runs the candidate rule of pislam_match_hamming_epipolar_batch's
// contract on each (pem::f_ok, pem::line, pem::near_line, pem::in_disc) and prints the line and the verdicts.
// tests/test_match_epipolar.py compares the words with its numpy restatement of the header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/epipolar_host_check.cpp -o epipolar_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   epipolar_host_check cases.txt        (or the cases on standard input)
// One element per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   nlevels qlevel tlevel  qobs[3] tobs[3]  f12[9] epipole[2]  level_sigma2[nlevels] level_scale[nlevels]  chi2 epipole_r2
// One line of output per element:
//   candidate near_line in_disc  a b c den
// (near_line and in_disc are 0 and the line four zeros when f12 is not finite or a level is not below nlevels; in_disc is
// the disc test alone, whatever the two keypoints are.)
#include <vector>
#include "hex_words.h"
#include "pislam_epipolar_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int elements = 0;
  for (;;) {
    int nlevels, ql, tl;
    const int got = fscanf(f, "%d %d %d", &nlevels, &ql, &tl);
    if (got == EOF) break;
    if (got != 3 || nlevels < 1 || nlevels > pem::MAX_LEVELS || ql < 0 || ql > 255 || tl < 0 || tl > 255)
      return fprintf(stderr, "element %d: bad header\n", elements), 2;
    // heap copies of exactly the sizes the procedure may touch: a read past them is an ASan report
    std::vector<int32_t> qobs(3), tobs(3);
    std::vector<float> F(9), ep(2), sg((size_t)nlevels), ls((size_t)nlevels);
    float par[2];
    bool ok = true;
    for (auto *o : {&qobs, &tobs})
      for (auto &v : *o) {
        long long q;
        ok = ok && fscanf(f, "%lld", &q) == 1 && q >= INT32_MIN && q <= INT32_MAX;
        v = (int32_t)q;
      }
    for (auto *a : {&F, &ep, &sg, &ls})
      for (auto &v : *a) ok = ok && rd_f32(f, &v);
    for (auto &v : par) ok = ok && rd_f32(f, &v);
    if (!ok) return fprintf(stderr, "element %d: truncated\n", elements), 2;
    pem::Tables tab{};
    tab.nlevels = nlevels;
    for (int l = 0; l < nlevels; l++) tab.level_sigma2[l] = sg[(size_t)l], tab.level_scale[l] = ls[(size_t)l];
    const pem::Params prm{par[0], par[1]};
    pem::Line ln{0.0f, 0.0f, 0.0f, 0.0f};
    bool cand = false, near = false, disc = false;
    if (pem::f_ok(F.data()) && ql < nlevels && tl < nlevels) {
      ln = pem::line(F.data(), pem::px(qobs[0]), pem::px(qobs[1]));
      const float u2 = pem::px(tobs[0]), v2 = pem::px(tobs[1]);
      const float lb = pem::line_bound(prm, tab, tl), db = pem::disc_bound(prm, tab, tl);
      near = pem::near_line(ln, u2, v2, lb);
      disc = pem::in_disc(ep[0], ep[1], u2, v2, db);
      cand = pem::candidate(ln, pem::mono(qobs[2]), ep[0], ep[1], u2, v2, pem::mono(tobs[2]), lb, db);
    }
    printf("%d %d %d", cand ? 1 : 0, near ? 1 : 0, disc ? 1 : 0);
    pr_f32(ln.a), pr_f32(ln.b), pr_f32(ln.c), pr_f32(ln.den);
    printf("\n");
    elements++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
