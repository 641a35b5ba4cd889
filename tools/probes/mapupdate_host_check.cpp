// Host check of the map-point update's rules (pislam_amd/csrc/pislam_mapupdate_math.h, shared with the kernels), on the
// CPU only: reads maps, runs pislam_map_points_update_batch's whole procedure for each serially (pmu::host_map) and
// writes all seven outputs.  tests/test_map_points_update.py compares the words with its restatement of the header
// comment.
//   g++ -std=c++17 -O1 -ffp-contract=off -I pislam_amd/csrc tools/probes/mapupdate_host_check.cpp -o mapupdate_host_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined ...   (the same)
//   mapupdate_host_check cases.bin out.bin
// Both files are little-endian 32-bit words; a float travels as its bit pattern.  cases.bin: the number of maps, then
// per map
//   nlevels nk kf_stride count stride npt pt_stride has_desc has_ref level_scale[nlevels]
//   obs_pt[stride] obs_kf[stride] obs_level[stride] (obs_desc[stride][8] if has_desc) poses[kf_stride][12]
//   xw[pt_stride][3] (ref[pt_stride] if has_ref)
// (nk, count and npt as the call is given them: they may be out of range, which is what the call has to refuse;
// the strides and the table within the call's limits.)  out.bin, per map:
//   status nobs[pt_stride] first[pt_stride] pt_status[pt_stride] normal[pt_stride][3] drange[pt_stride][2]
//   (desc[pt_stride][8] if has_desc)
// where a word that the call does not write holds 0x5A5A5A5A (a byte of pt_status: 0x5A).
#include <stdio.h>
#include <string.h>
#include <vector>
#include "pislam_mapupdate_math.h"

static const uint32_t SENTINEL = 0x5A5A5A5Au;

static bool rd(FILE *f, void *v, size_t n) { return fread(v, 4, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: mapupdate_host_check cases.bin out.bin\n"), 2;
  FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
  if (!f || !g) return fprintf(stderr, "cannot open %s\n", f ? argv[2] : argv[1]), 2;
  int32_t maps;
  if (!rd(f, &maps, 1) || maps < 0) return fprintf(stderr, "bad file header\n"), 2;
  for (int32_t m = 0; m < maps; m++) {
    int32_t h[9];
    if (!rd(f, h, 9)) return fprintf(stderr, "map %d: truncated header\n", m), 2;
    const int64_t nlevels = h[0], nk = h[1], ks = h[2], count = h[3], stride = h[4], npt = (uint32_t)h[5], ps = h[6];
    if (nlevels < 1 || nlevels > pmu::MAX_LEVELS || ks < 1 || ks > pmu::MAX_KF || stride < 1 || ps < 1)
      return fprintf(stderr, "map %d: bad header\n", m), 2;
    pmu::Tables tab{};
    tab.nlevels = (int32_t)nlevels;
    if (!rd(f, tab.level_scale, (size_t)nlevels)) return fprintf(stderr, "map %d: truncated table\n", m), 2;
    // heap copies of exactly the sizes the procedure may touch: a read or write past them is an ASan report
    std::vector<int32_t> pt((size_t)stride), word((size_t)(stride > ps ? stride : ps));
    std::vector<uint16_t> kf((size_t)stride), ref;
    std::vector<uint8_t> level((size_t)stride);
    std::vector<uint32_t> od;
    std::vector<float> poses((size_t)ks * 12), xw((size_t)ps * 3);
    bool ok = rd(f, pt.data(), pt.size()) && rd(f, word.data(), (size_t)stride);
    for (size_t i = 0; i < kf.size(); i++) kf[i] = (uint16_t)word[i];
    ok = ok && rd(f, word.data(), (size_t)stride);
    for (size_t i = 0; i < level.size(); i++) level[i] = (uint8_t)word[i];
    if (h[7]) od.resize((size_t)stride * pmu::WORDS), ok = ok && rd(f, od.data(), od.size());
    ok = ok && rd(f, poses.data(), poses.size()) && rd(f, xw.data(), xw.size());
    if (h[8]) {
      ref.resize((size_t)ps);
      ok = ok && rd(f, word.data(), (size_t)ps);
      for (size_t i = 0; i < ref.size(); i++) ref[i] = (uint16_t)word[i];
    }
    if (!ok) return fprintf(stderr, "map %d: truncated\n", m), 2;
    pmu::Map M;
    M.obs_pt = pt.data(), M.obs_kf = kf.data(), M.obs_level = level.data(), M.obs_desc = h[7] ? od.data() : nullptr;
    M.poses = poses.data(), M.xw = xw.data(), M.ref = h[8] ? ref.data() : nullptr;
    M.count = count, M.stride = stride, M.nk = nk, M.kf_stride = ks, M.npt = npt, M.pt_stride = ps;
    std::vector<uint32_t> normal((size_t)ps * 3, SENTINEL), drange((size_t)ps * 2, SENTINEL);
    std::vector<uint32_t> desc(h[7] ? (size_t)ps * pmu::WORDS : 0, SENTINEL);
    std::vector<int32_t> nobs((size_t)ps, (int32_t)SENTINEL), first((size_t)ps, (int32_t)SENTINEL);
    std::vector<uint8_t> pt_status((size_t)ps, 0x5A);
    int32_t status;
    static_assert(sizeof(float) == 4, "a float is a 32-bit word");
    pmu::host_map(M, tab, (float *)normal.data(), (float *)drange.data(), h[7] ? desc.data() : nullptr, nobs.data(),
                  first.data(), pt_status.data(), &status);
    std::vector<uint32_t> out;
    out.push_back((uint32_t)status);
    out.insert(out.end(), nobs.begin(), nobs.end());
    out.insert(out.end(), first.begin(), first.end());
    out.insert(out.end(), pt_status.begin(), pt_status.end());
    out.insert(out.end(), normal.begin(), normal.end());
    out.insert(out.end(), drange.begin(), drange.end());
    out.insert(out.end(), desc.begin(), desc.end());
    if (fwrite(out.data(), 4, out.size(), g) != out.size()) return fprintf(stderr, "cannot write\n"), 2;
  }
  fclose(f);
  return fclose(g) ? 2 : 0;
}
