// Host check of the pyramid build's planner (pislam_amd/csrc/pislam_prep_plan.h: pp::layout, pp::make_build_plan), on
// the CPU only.  A few thousand random and edge level tables; what the planner accepts is checked against brute-force
// restatements that use none of the header's helpers: the level slots, the workgroup ranges and band counters of the
// one-launch build as pp::k_bilinear_chain decodes them, the counter words, the 4-block rule and the margins.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pislam_amd/csrc tools/probes/prep_host_check.cpp -o tools/probes/_bin/prep_host_check && tools/probes/_bin/prep_host_check
// --dump prints one line per fixed case (tests/golden/build_plans.json, tests/test_build_plan_golden.py);
// --random N SEED prints the same line for N random tables.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "pislam_prep_plan.h"

struct Case {
  std::string name;
  int nlevels = 1;
  int32_t steps[16] = {0};
  pislam_level levels[16];
  int frame_vstep = 0, batch = 1, vstep = 0, rows = 0, flags = PISLAM_BUILD_BLUR;
  size_t frame_stride = 0, pyramid_stride = 0;
  unsigned pyramids_mod16 = 0;
  bool chain_wanted = true, host_pointers = false;
};

// what a call answers: the dump line
struct Record {
  const char *refusal = nullptr;
  bool chain = false;
  unsigned grid = 0, quads = 0;        // quads: bit l = the reduction of level l takes the 4-block kernel
  size_t words = 0;
  uint64_t zhash = 0, chash = 0;
};

static uint64_t fnv1a(const void *p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}

static Case make_case(const char *name, int width, int height, std::vector<int> steps, int batch) {
  Case c;
  c.name = name;
  c.nlevels = (int)steps.size() + 1;
  for (size_t i = 0; i < steps.size(); i++) c.steps[i] = steps[i];
  int32_t vstep = 0, rows = 0;
  if (pp::layout(width, height, c.nlevels, c.steps, 0, c.levels, &vstep, &rows) != PISLAM_OK) {
    fprintf(stderr, "%s: layout refused\n", name);
    exit(2);
  }
  c.vstep = vstep, c.rows = rows, c.batch = batch;
  c.frame_vstep = width, c.frame_stride = (size_t)width * height, c.pyramid_stride = (size_t)rows * vstep;
  return c;
}

static Record plan_case(const Case &c, pp::BuildPlan *out = nullptr) {
  Record r;
  static const uint8_t some = 0;
  r.refusal = pp::check_build_call(c.nlevels, c.steps, c.levels, &some, &some, c.batch, c.flags);
  if (!r.refusal && c.host_pointers) r.refusal = pp::HOST_POINTERS;
  if (r.refusal) return r;
  const pp::BuildPlan P = pp::make_build_plan(c.nlevels, c.steps, c.levels, c.frame_vstep, c.frame_stride, c.batch, c.vstep, c.rows,
                                              c.pyramid_stride, c.flags, c.pyramids_mod16, c.chain_wanted);
  if (out) *out = P;
  r.refusal = P.refusal;
  if (r.refusal) return r;
  r.chain = P.chain, r.grid = P.chain_grid, r.words = P.chain_words;
  for (int l = 0; l + 1 < c.nlevels; l++) r.quads |= (unsigned)P.red[l].quad << l;
  r.zhash = fnv1a(&P.Z, sizeof(P.Z)), r.chash = fnv1a(&P.C, sizeof(P.C));
  return r;
}

static void print_record(const Case &c, const Record &r) {
  if (r.refusal) printf("%s: %s\n", c.name.c_str(), r.refusal);
  else
    printf("%s: ok chain=%d grid=%u words=%zu quads=%x Z=%016llx C=%016llx\n", c.name.c_str(), (int)r.chain, r.grid, r.words, r.quads,
           (unsigned long long)r.zhash, (unsigned long long)r.chash);
}

static std::vector<Case> fixed_cases() {
  std::vector<Case> v;
  const std::vector<int> s7 = {2, 1, 2, 2, 1, 2, 2};
  v.push_back(make_case("720p-64", 1280, 720, s7, 64));
  v.push_back(make_case("vga-5", 640, 480, s7, 5));
  v.push_back(make_case("333x251-3", 333, 251, {1, 2, 1}, 3));
  v.push_back(make_case("1080p-2", 1920, 1080, {2, 2, 1, 2}, 2));
  v.push_back(make_case("48x40-9", 48, 40, {2, 1, 2}, 9));          // (16-byte loads of three 16-blocks need 64 columns: per level)
  v.push_back(make_case("64x40-9", 64, 40, {2, 1, 2}, 9));          // the smallest one-launch build, crossing the eight-frame group
  v.push_back(make_case("one-level", 48, 40, {}, 1));
  v.push_back(make_case("two-levels", 48, 40, {1}, 1));
  v.push_back(make_case("sixteen-levels", 1280, 720, std::vector<int>(15, 1), 1));
  for (int batch : {1, 8, 9, 65}) v.push_back(make_case(("vga-batch-" + std::to_string(batch)).c_str(), 640, 480, {2, 1, 2}, batch));
  v.push_back(make_case("40x40-quad-loads-do-not-fit", 40, 40, {2, 2, 1}, 2));
  Case c = make_case("chain-not-wanted", 640, 480, {2, 1, 2}, 4);
  c.chain_wanted = false;
  v.push_back(c);
  c = make_case("margins-clean", 640, 480, {2, 1, 2}, 4);
  c.flags = PISLAM_BUILD_BLUR | PISLAM_BUILD_MARGINS_CLEAN;
  v.push_back(c);
  c = make_case("margins-checked", 640, 480, {2, 1, 2}, 4);
  c.flags = PISLAM_BUILD_MARGINS_CLEAN | PISLAM_BUILD_CHECK_MARGINS;
  v.push_back(c);
  c = make_case("pyramids-misaligned", 640, 480, {2, 1, 2}, 4);
  c.pyramids_mod16 = 4;
  v.push_back(c);
  c = make_case("vstep-misaligned", 640, 480, {2, 1, 2}, 4);
  c.vstep += 4, c.pyramid_stride = (size_t)c.rows * c.vstep;
  v.push_back(c);
  c = make_case("stride-misaligned", 640, 480, {2, 1, 2}, 4);
  c.pyramid_stride += 2;
  v.push_back(c);
  // one case per refusal, at 48 x 40 (tests/test_prep.py makes the same calls on the device)
  c = make_case("refused-flags", 48, 40, {2, 1, 2}, 2);
  c.flags = 8;
  v.push_back(c);
  c = make_case("refused-batch", 48, 40, {2, 1, 2}, 2);
  c.batch = 0;
  v.push_back(c);
  c = make_case("refused-host-pointers", 48, 40, {2, 1, 2}, 2);
  c.host_pointers = true;
  v.push_back(c);
  c = make_case("refused-level-does-not-fit", 48, 40, {2, 1, 2}, 2);
  c.vstep = 32;
  v.push_back(c);
  c = make_case("refused-block-overrun", 48, 40, {2, 1, 2}, 2);
  c.levels[2].row0 -= 8;
  v.push_back(c);
  c = make_case("refused-frame-buffer", 48, 40, {2, 1, 2}, 2);
  c.frame_vstep = 47;
  v.push_back(c);
  return v;
}

// A random table: mostly what pp::layout makes of a random size and step list, then, in about half of them, one field disturbed.
static Case random_case(std::mt19937 &rng, int i) {
  auto U = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  for (;;) {
    Case c;
    c.name = "random-" + std::to_string(i);
    c.nlevels = U(0, 9) ? U(1, 8) : U(9, 16);
    for (int l = 0; l + 1 < c.nlevels; l++) c.steps[l] = U(1, 2);
    const int big = U(0, 19) == 0;
    const int width = U(3, big ? 2000 : 400), height = U(3, big ? 1200 : 300);
    int32_t vstep = 0, rows = 0;
    if (pp::layout(width, height, c.nlevels, c.steps, U(0, 3) ? 0 : U(1, 2048), c.levels, &vstep, &rows) != PISLAM_OK) continue;
    c.vstep = vstep, c.rows = rows, c.batch = U(0, 5) ? U(1, 20) : U(1, 300);
    c.frame_vstep = width + (U(0, 2) ? 0 : U(0, 64)), c.frame_stride = (size_t)c.frame_vstep * height + (U(0, 2) ? 0 : U(0, 100));
    c.pyramid_stride = (size_t)rows * vstep + (U(0, 2) ? 0 : 16 * U(0, 8));
    c.flags = U(0, 7);
    c.chain_wanted = U(0, 3) != 0;
    const int l = U(0, c.nlevels - 1);
    switch (U(0, 29)) {
      case 0: c.vstep += U(-20, 20); break;
      case 1: c.rows += U(-20, 20); break;
      case 2: c.levels[l].row0 += U(-20, 20); break;
      case 3: c.levels[l].col0 = U(0, 1); break;
      case 4: c.levels[l].width += U(-9, 9), c.levels[l].height += U(-9, 9); break;
      case 5: c.frame_vstep -= U(0, 3); break;
      case 6: c.frame_stride -= (size_t)U(0, 3); break;
      case 7: c.pyramid_stride += (size_t)U(-3, 40); break;
      case 8: c.pyramids_mod16 = (unsigned)U(0, 15); break;
      case 9: c.steps[l] = U(-1, 4); break;
      case 10: c.flags = U(-2, 40); break;
      case 11: c.batch = U(-1, 1); break;
      case 12: c.host_pointers = true; break;
      case 13: c.vstep = (c.vstep + 16 * U(0, 3)) | (U(0, 1) ? 4 : 8); break;
      default: break;
    }
    if (c.vstep <= 0 || c.rows <= 0 || c.levels[l].width <= 0 || c.levels[l].height <= 0 || c.levels[l].row0 < 0) continue;
    return c;
  }
}

// ---- the brute-force restatements ----
static const int BN[3] = {0, 8, 16}, BM[3] = {0, 7, 13};
static int code(int step) { return step == 1 ? 1 : 2; }
static int count_blocks(int x, int n) {        // blocks of n that cover x pixels
  int b = 0;
  for (int covered = 0; covered < x; covered += n) b++;
  return b;
}

#define EXPECT(cond)                                                               \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      printf("FAIL %s: %s (line %d)\n", c.name.c_str(), #cond, __LINE__);          \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

// the table pp::layout made for (width, height, steps)
static int check_layout(const Case &c, int width, int height) {
  int w = width, h = height;
  for (int l = 0; l < c.nlevels; l++) {
    const pislam_level &L = c.levels[l];
    const int end = l + 1 < c.nlevels ? c.levels[l + 1].row0 : c.rows;
    EXPECT(L.width == w && L.height == h && L.col0 == 0 && L.row0 >= 0);
    EXPECT(l == 0 ? L.row0 == 0 : L.row0 >= c.levels[l - 1].row0 + c.levels[l - 1].height);   // slots do not overlap
    EXPECT(L.row0 + h <= end && w <= c.vstep);
    if (l + 1 < c.nlevels) {                                     // the padding the next reduction reads
      const int n = BN[c.steps[l]], m = BM[c.steps[l]];
      EXPECT(L.row0 + count_blocks(h, n) * n <= end && count_blocks(w, n) * n <= c.vstep);
      EXPECT(c.levels[l + 1].row0 + count_blocks(h, n) * m <= (l + 2 < c.nlevels ? c.levels[l + 2].row0 : c.rows));   // every block it writes
      EXPECT(count_blocks(w, n) * m <= c.vstep);
      w = (int)((long long)w * m / n), h = (int)((long long)h * m / n);
    }
  }
  EXPECT(c.vstep % 16 == 0);
  return 0;
}

// a plan the planner accepted
static int check_plan(const Case &c, const pp::BuildPlan &P) {
  const int nl = c.nlevels;
  unsigned quads_all = 1;
  for (int l = 0; l + 1 < nl; l++) {
    const int n = BN[code(c.steps[l])], m = BM[code(c.steps[l])];
    const pp::ReductionPlan &R = P.red[l];
    const int nbx = count_blocks(c.levels[l].width, n), nby = count_blocks(c.levels[l].height, n);
    EXPECT(R.width == c.levels[l].width && R.height == c.levels[l].height && R.ow == nbx * m && R.oh == nby * m);
    EXPECT(R.src_ofs == (size_t)c.levels[l].row0 * c.vstep && R.dst_ofs == (size_t)c.levels[l + 1].row0 * c.vstep);
    // the 4-block kernel: aligned 16-byte loads, dword stores, and the last group of four blocks ends inside the row
    int last_load_end = 0;
    for (int bx = 0; bx < nbx; bx += 4) last_load_end = (bx + 4) * n;
    const bool quad = (c.pyramids_mod16 + R.src_ofs) % 16 == 0 && (c.pyramids_mod16 + R.dst_ofs) % 4 == 0 && c.vstep % 16 == 0 &&
                      c.pyramid_stride % 16 == 0 && last_load_end <= c.vstep;
    EXPECT(R.quad == quad);
    quads_all &= quad;
    // what it writes stays inside the destination's slot
    EXPECT(R.ow <= c.vstep && c.levels[l + 1].row0 + R.oh <= (l + 2 < nl ? c.levels[l + 2].row0 : c.rows));
  }
  if (P.margins) {
    EXPECT(P.Z.nlevels == nl && P.Z.vstep == c.vstep);
    for (int l = 0; l < nl; l++) {
      const int slot = (l + 1 < nl ? c.levels[l + 1].row0 : c.rows) - c.levels[l].row0;
      EXPECT(P.Z.row0[l] == c.levels[l].row0 && P.Z.slot_rows[l] == slot && slot > 0 && P.Z.row0[l] >= 0 && P.Z.row0[l] + slot <= c.rows);
      EXPECT(P.Z.ww[l] == (l ? P.red[l - 1].ow : c.levels[0].width) && P.Z.wh[l] == (l ? P.red[l - 1].oh : c.levels[0].height));
      // The rectangle a reduction writes stays inside the slot, and so do the margins: the kernel clips them to the slot
      // and the row.  (Level 0 is as tall as the caller's table says: the build only asks that it ends inside the buffer.)
      EXPECT(P.Z.ww[l] <= c.vstep && (l ? P.Z.wh[l] <= slot : P.Z.row0[0] + P.Z.wh[0] <= c.rows));    }
  }
  EXPECT(!P.chain || (c.chain_wanted && nl >= 3 && quads_all));   // eligibility implies the 4-block kernel on every level
  if (!P.chain) return 0;
  const pp::ChainPlan &C = P.C;
  const int groups = count_blocks(c.batch, 8);
  EXPECT(C.nlevels == nl && C.vstep == c.vstep && C.batch == c.batch && C.groups == groups && C.row0[0] == c.levels[0].row0);
  long long grid = 0;
  int bands = 0;
  for (int l = 1; l < nl; l++) {
    const int n = BN[code(c.steps[l - 1])], m = BM[code(c.steps[l - 1])];
    const int nq = count_blocks(count_blocks(c.levels[l - 1].width, n), 4), oh = count_blocks(c.levels[l - 1].height, n) * m;
    EXPECT(C.kind[l] == c.steps[l - 1] && (C.kind[l] == 1) == (n == 8) && C.row0[l] == c.levels[l].row0);
    EXPECT(C.sw[l] == c.levels[l - 1].width && C.sh[l] == c.levels[l - 1].height && C.nq[l] == nq && C.oh[l] == oh);
    EXPECT(C.wg0[l] == grid && C.wg0[l] % 8 == 0 && (l == 1 || C.wg0[l] > C.wg0[l - 1]));
    // the kernel's decoding of this level's workgroups: every (frame of a whole group, chunk of 256 items) exactly once
    const int wpf = C.wpf[l];
    EXPECT(wpf == count_blocks(nq * oh, 256));
    std::vector<uint8_t> seen((size_t)8 * groups * wpf, 0);
    for (long long wg = C.wg0[l]; wg < C.wg0[l] + 8LL * groups * wpf; wg++) {
      const int b = (int)(wg - C.wg0[l]), rest = b >> 3, g = rest / wpf, chunk = rest - g * wpf, frame = 8 * g + (b & 7);
      EXPECT(g < groups && chunk * 256 < nq * oh && !seen[(size_t)frame * wpf + chunk]);
      seen[(size_t)frame * wpf + chunk] = 1;
    }
    grid += 8LL * groups * wpf;
    // every output row in exactly one band
    EXPECT(C.band0[l] == bands);
    std::vector<int> rows_of_band;
    for (int y = 0; y < oh; y++) {
      const size_t band = (size_t)(y / pp::CH_BAND);
      if (band == rows_of_band.size()) rows_of_band.push_back(0);
      EXPECT(band + 1 == rows_of_band.size());
      rows_of_band[band]++;
    }
    for (size_t b = 0; b < rows_of_band.size(); b++) EXPECT(rows_of_band[b] == std::min(pp::CH_BAND, oh - (int)b * pp::CH_BAND));
    bands += (int)rows_of_band.size();
  }
  EXPECT(C.wg0[nl] == grid && P.chain_grid == grid && grid <= 0x3fffffff && C.bands_per_frame == bands);
  // the highest counter word the kernel addresses: the frames' band counters, then one 128-byte line each for
  // [fault, shards complete, CH_SHARDS shard counters, one word per frame of a whole group]
  size_t tail = 0;
  while (tail < (size_t)c.batch * bands) tail += pp::CH_LINE;
  EXPECT((size_t)(c.batch - 1) * bands + (bands - 1) < tail);
  const size_t highest = tail + (size_t)(2 + pp::CH_SHARDS + 8 * groups - 1) * pp::CH_LINE;
  EXPECT(P.chain_words > highest && P.chain_words == highest + pp::CH_LINE);
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "--dump")) {
    for (const Case &c : fixed_cases()) print_record(c, plan_case(c));
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "--random")) {
    std::mt19937 rng((unsigned)atoi(argv[3]));
    for (int i = 0, n = atoi(argv[2]); i < n; i++) {
      const Case c = random_case(rng, i);
      print_record(c, plan_case(c));
    }
    return 0;
  }
  int bad = 0, accepted = 0, refused = 0, chains = 0, layouts = 0;
  std::mt19937 rng(1);
  // layouts: every size near a block edge, and random ones
  for (int i = 0; i < 3000; i++) {
    auto U = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    std::vector<int> steps(U(0, 15));
    for (int &s : steps) s = U(1, 2);
    const int width = i < 400 ? 3 + i % 40 : U(3, 2000), height = i < 400 ? 3 + i / 40 * 3 : U(3, 1200);
    Case c;
    c.name = "layout " + std::to_string(width) + "x" + std::to_string(height);
    c.nlevels = (int)steps.size() + 1;
    for (size_t k = 0; k < steps.size(); k++) c.steps[k] = steps[k];
    int32_t vstep = 0, rows = 0;
    if (pp::layout(width, height, c.nlevels, c.steps, 0, c.levels, &vstep, &rows) != PISLAM_OK) continue;
    c.vstep = vstep, c.rows = rows;
    bad += check_layout(c, width, height);
    layouts++;
  }
  std::vector<Case> cases = fixed_cases();
  for (int i = 0; i < 6000; i++) cases.push_back(random_case(rng, i));
  for (const Case &c : cases) {
    pp::BuildPlan P;
    const Record r = plan_case(c, &P);
    if (r.refusal) {
      refused++;
      continue;
    }
    accepted++, chains += r.chain;
    bad += check_plan(c, P);
  }
  printf("%d layouts, %d plans accepted (%d as one launch), %d refused\n", layouts, accepted, chains, refused);
  printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
