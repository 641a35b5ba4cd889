// Host check of the reconstruction call's arithmetic (pislam_amd/csrc/pislam_recon_math.h, shared with the kernel), on
// the CPU only: reads pairs, runs pislam_two_view_reconstruct_batch's whole procedure serially (prm::host_pair) and
// prints every output word.  tests/test_two_view_reconstruct.py compares the words with its numpy restatement of the
// header comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/recon_host_check.cpp -o recon_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   recon_host_check cases.txt        (or the cases on standard input)
// One pair per line, whitespace separated; floats are hexadecimal bit patterns, the rest decimal integers:
//   ncand sigma_q8 cos_parallax cos_point min_good min_good_pct similar_pct parallax_rank has_mask n  cam[4]
//   cand[ncand][12]  then per match: x1_q8 y1_q8 x2_q8 y2_q8 mask
// (n is what the call makes of counts[b] and stride: already clamped.)  One line of output per pair:
//   best status ngood[8] npar[8] pose_out[12] point[n] as a string of 0 / 1 ("-" for n == 0) xw[n][3]
#include <vector>
#include "hex_words.h"
#include "pislam_recon_math.h"

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int pairs = 0;
  for (;;) {
    prm::Params P;
    int has_mask;
    long long n;
    const int got = fscanf(f, "%" SCNd32 " %" SCNd32, &P.ncand, &P.sigma_q8);
    if (got == EOF) break;
    bool ok = got == 2 && rd_f32(f, &P.cos_parallax) && rd_f32(f, &P.cos_point);
    ok = ok && fscanf(f, "%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %d %lld", &P.min_good, &P.min_good_pct,
                      &P.similar_pct, &P.parallax_rank, &has_mask, &n) == 6;
    if (!ok || !prm::params_ok(P) || n < 0 || n > prm::MAX_STRIDE) return fprintf(stderr, "pair %d: bad header\n", pairs), 2;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<float> cam(4), cand(12 * (size_t)P.ncand), xw(3 * (size_t)n);
    std::vector<int32_t> p1(2 * (size_t)n), p2(2 * (size_t)n);
    std::vector<uint8_t> mask((size_t)n), point((size_t)n);
    for (auto &v : cam) ok = ok && rd_f32(f, &v);
    for (auto &v : cand) ok = ok && rd_f32(f, &v);
    for (long long i = 0; ok && i < n; i++) {
      long long q[5];
      ok = fscanf(f, "%lld %lld %lld %lld %lld", &q[0], &q[1], &q[2], &q[3], &q[4]) == 5;
      if (!ok) break;
      p1[2 * (size_t)i] = (int32_t)q[0], p1[2 * (size_t)i + 1] = (int32_t)q[1];
      p2[2 * (size_t)i] = (int32_t)q[2], p2[2 * (size_t)i + 1] = (int32_t)q[3];
      mask[(size_t)i] = (uint8_t)q[4];
    }
    if (!ok) return fprintf(stderr, "pair %d: truncated\n", pairs), 2;
    prm::PairIn I;
    I.p1 = p1.data(), I.p2 = p2.data(), I.mask = has_mask ? mask.data() : nullptr, I.cam = cam.data();
    I.cand = cand.data(), I.n = (uint32_t)n;
    prm::PairOut O;
    prm::host_pair(I, P, &O, xw.data(), point.data());
    printf("%" PRId32 " %" PRIu32, O.best, O.status);
    for (int c = 0; c < prm::MAX_CAND; c++) printf(" %" PRIu32, O.ngood[c]);
    for (int c = 0; c < prm::MAX_CAND; c++) printf(" %" PRIu32, O.npar[c]);
    for (int i = 0; i < 12; i++) pr_f32(O.pose[i]);
    printf(" ");
    if (n == 0) printf("-");
    for (long long i = 0; i < n; i++) putchar(point[(size_t)i] ? '1' : '0');
    for (size_t i = 0; i < 3 * (size_t)n; i++) pr_f32(xw[i]);
    printf("\n");
    pairs++;
  }
  if (f != stdin) fclose(f);
  return 0;
}
