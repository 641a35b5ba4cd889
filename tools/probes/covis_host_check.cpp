// Host check of the covisibility graph's rules (pislam_amd/csrc/pislam_covis_math.h, shared with the kernels), on the
// CPU only: reads maps, runs pislam_covisibility_batch's whole procedure for each serially (pcv::host_map) and writes
// all seven outputs.  tests/test_covisibility.py compares the words with its restatement of the header comment.
//   g++ -std=c++17 -O1 -I pislam_amd/csrc tools/probes/covis_host_check.cpp -o covis_host_check
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   covis_host_check cases.bin out.bin
// Both files are little-endian int32 words.  cases.bin: the number of maps, then per map
//   min_weight cull_min_observers cull_level_slack nk kf_stride count stride nb_stride has_level has_mask
//   obs_pt[stride] obs_kf[stride] (obs_level[stride] if has_level) (cull_mask[stride] if has_mask)
// (nk and count as the call is given them: they may be out of range, which is what the call has to refuse; kf_stride,
// stride and nb_stride within the call's limits.)  out.bin, per map:
//   status nb_count[kf_stride] parent[kf_stride] kf_points[kf_stride] kf_redundant[kf_stride]
//   nb_idx[kf_stride][nb_stride] nb_weight[kf_stride][nb_stride]
// where a word of nb_idx or nb_weight that the call does not write holds 0x5A5A5A5A.
#include <stdio.h>
#include <vector>
#include "pislam_covis_math.h"

static const int32_t SENTINEL = 0x5A5A5A5A;

static bool rd(FILE *f, int32_t *v, size_t n) { return fread(v, sizeof(int32_t), n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: covis_host_check cases.bin out.bin\n"), 2;
  FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
  if (!f || !g) return fprintf(stderr, "cannot open %s\n", f ? argv[2] : argv[1]), 2;
  int32_t maps;
  if (!rd(f, &maps, 1) || maps < 0) return fprintf(stderr, "bad file header\n"), 2;
  for (int32_t m = 0; m < maps; m++) {
    int32_t h[10];
    if (!rd(f, h, 10)) return fprintf(stderr, "map %d: truncated header\n", m), 2;
    const pcv::Params P{h[0], h[1], h[2]};
    const int64_t nk = h[3], ks = h[4], count = h[5], stride = h[6], nbs = h[7];
    if (P.min_weight < 1 || P.cull_min_observers < 1 || P.cull_level_slack < 0 || P.cull_level_slack > 255 || ks < 1 ||
        ks > pcv::MAX_KF || stride < 1 || nbs < 1 || nbs > ks)
      return fprintf(stderr, "map %d: bad header\n", m), 2;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<int32_t> pt((size_t)stride), word((size_t)stride);
    std::vector<uint16_t> kf((size_t)stride);
    std::vector<uint8_t> level, mask;
    bool ok = rd(f, pt.data(), pt.size()) && rd(f, word.data(), word.size());
    for (size_t i = 0; i < kf.size(); i++) kf[i] = (uint16_t)word[i];
    for (std::vector<uint8_t> *v : {&level, &mask}) {
      if (!h[v == &level ? 8 : 9]) continue;
      ok = ok && rd(f, word.data(), word.size());
      v->resize((size_t)stride);
      for (size_t i = 0; i < v->size(); i++) (*v)[i] = (uint8_t)word[i];
    }
    if (!ok) return fprintf(stderr, "map %d: truncated\n", m), 2;
    pcv::Map M;
    M.obs_pt = pt.data(), M.obs_kf = kf.data(), M.obs_level = h[8] ? level.data() : nullptr;
    M.cull_mask = h[9] ? mask.data() : nullptr, M.count = count, M.stride = stride, M.nk = nk, M.kf_stride = ks;
    std::vector<uint16_t> nb_idx((size_t)(ks * nbs)), parent((size_t)ks);
    std::vector<int32_t> nb_weight((size_t)(ks * nbs), SENTINEL), nb_count((size_t)ks), pts((size_t)ks), red((size_t)ks);
    int32_t status;
    pcv::host_map(M, P, (size_t)nbs, nb_idx.data(), nb_weight.data(), nb_count.data(), parent.data(), pts.data(), red.data(),
                  &status);
    std::vector<int32_t> out;
    out.push_back(status);
    out.insert(out.end(), nb_count.begin(), nb_count.end());
    out.insert(out.end(), parent.begin(), parent.end());
    out.insert(out.end(), pts.begin(), pts.end());
    out.insert(out.end(), red.begin(), red.end());
    for (int64_t k = 0; k < ks; k++)      // (a row's written prefix is min(nb_count, nb_stride) long)
      for (int64_t r = 0; r < nbs; r++)
        out.push_back(r < nb_count[(size_t)k] ? (int32_t)nb_idx[(size_t)(k * nbs + r)] : SENTINEL);
    out.insert(out.end(), nb_weight.begin(), nb_weight.end());
    if (fwrite(out.data(), sizeof(int32_t), out.size(), g) != out.size()) return fprintf(stderr, "cannot write\n"), 2;
  }
  fclose(f);
  return fclose(g) ? 2 : 0;
}
