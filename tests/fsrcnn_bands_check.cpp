// Stand-alone check of FSRCNN's band plan (sharkshark-4k_amd/csrc/fsrcnn_bands.h): the launcher's plan and the kernels' walk, run on the host
// over a sweep of shapes.  Built with AddressSanitizer and UBSan and run by tests/test_fsrcnn_bands_cpu.py; no HIP, no Python extension.
#include "../sharkshark-4k_amd/csrc/fsrcnn_bands.h"
#include <cstdio>
#include <vector>

namespace fb = ss4k::fs_bands;

static int g_fail = 0;
static long g_walks = 0;

#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                        \
  } while (0)

// Walks band indices [0, count + 3) as a kernel does and checks: every (plane, row) exactly once - the segments, in band order, must tile the
// stacked rows 0 .. planes * h without a gap or an overlap - every segment inside one plane, nothing at or past `count`; tall: every band but
// the last has tall_rpb rows
static void walk_all(int planes, int h, int bands, int tall_rpb, int count, const char* what) {
  ++g_walks;
  long pos = 0;   // the stacked row (plane * h + y) the next segment must start at
  for (int u = 0; u < count + 3; ++u) {
    fb::Walk k = fb::first(u, planes, h, bands, tall_rpb);
    if (u >= count) { CHECK(k.empty(), "%s planes %d h %d bands %d rpb %d: band %d of %d visits rows", what, planes, h, bands, tall_rpb, u, count); continue; }
    int rows = 0, segments = 0;
    if (!k.empty()) do {
      ++segments;
      const bool inside = k.plane >= 0 && k.plane < planes && 0 <= k.ylo && k.ylo < k.yhi && k.yhi <= h;
      CHECK(inside, "%s planes %d h %d bands %d rpb %d band %d: segment plane %d rows [%d, %d)", what, planes, h, bands, tall_rpb, u, k.plane, k.ylo, k.yhi);
      if (!inside) return;
      CHECK((long)k.plane * h + k.ylo == pos, "%s planes %d h %d bands %d rpb %d band %d: segment plane %d rows [%d, %d) after stacked row %ld", what, planes, h, bands,
            tall_rpb, u, k.plane, k.ylo, k.yhi, pos);
      pos = (long)k.plane * h + k.yhi;
      rows += k.yhi - k.ylo;
    } while (k.next(h));
    if (tall_rpb > 0) CHECK(u == count - 1 ? (rows >= 1 && rows <= tall_rpb) : rows == tall_rpb, "%s planes %d h %d rpb %d: band %d of %d has %d rows", what, planes, h, tall_rpb, u, count, rows);
    else CHECK(segments <= 1, "%s planes %d h %d bands %d: classic band %d has %d segments", what, planes, h, bands, u, segments);
  }
  CHECK(pos == (long)planes * h, "%s planes %d h %d bands %d rpb %d: the walk ends at stacked row %ld of %ld", what, planes, h, bands, tall_rpb, pos, (long)planes * h);
}

int main() {
  struct Stage { const char* name; int min_rows, slots_per_cu; };
  const Stage stages[3] = {{"fp16 maps", fb::MAPS_MIN_ROWS, fb::MAPS_SLOTS_PER_CU}, {"fp32-grade maps", fb::MAPS_MIN_ROWS, fb::MAPS_SLOTS_PER_CU},
                           {"tail", fb::TAIL_MIN_ROWS, fb::TAIL_SLOTS_PER_CU}};
  std::vector<int> hs;
  for (int h = 1; h <= 40; ++h) hs.push_back(h);
  for (int h : {45, 70, 180, 720}) hs.push_back(h);
  for (int planes = 1; planes <= 13; ++planes)
    for (int h : hs) {
      for (int bands = 1; bands <= h + 2; ++bands) walk_all(planes, h, bands, 0, planes * bands, "classic");
      for (int strips : {1, 2, 23, 46})
        for (int num_cu : {1, 8, 256, 304})
          for (const Stage& s : stages) {
            const fb::Plan tall = fb::plan(planes, h, strips, s.min_rows, s.slots_per_cu * num_cu, false);
            const long rows = (long)planes * h;
            CHECK(tall.tall_rpb >= 1 && tall.bands == (rows + tall.tall_rpb - 1) / tall.tall_rpb && tall.band_count(planes) == tall.bands,
                  "%s planes %d h %d strips %d cu %d: rpb %d bands %d", s.name, planes, h, strips, num_cu, tall.tall_rpb, tall.bands);
            if (tall.tall_rpb >= 1) walk_all(planes, h, tall.bands, tall.tall_rpb, tall.bands, s.name);
            // the classic plan of the same stage: a band count of the sweep above (walked there), one round of units
            const fb::Plan cl = fb::plan(planes, h, strips, s.min_rows, s.slots_per_cu * num_cu, true);
            CHECK(cl.tall_rpb == 0 && cl.bands >= 1 && cl.bands <= h + 2 && cl.band_count(planes) == planes * cl.bands,
                  "%s planes %d h %d strips %d cu %d: classic bands %d", s.name, planes, h, strips, num_cu, cl.bands);
          }
    }
  // the anchors of the kernels' comments: 12 planes of 720 x 1280 at 256 CUs
  const fb::Plan m = fb::plan(12, 720, 23, fb::MAPS_MIN_ROWS, fb::MAPS_SLOTS_PER_CU * 256, false);   // fp16 maps: 23 strips of 56 columns
  CHECK(m.tall_rpb == 197 && m.bands == 44 && m.bands * 23 == 1012, "fp16 maps anchor: rpb %d bands %d", m.tall_rpb, m.bands);
  const fb::Plan t = fb::plan(12, 720, 46, fb::TAIL_MIN_ROWS, fb::TAIL_SLOTS_PER_CU * 256, false);   // x2 tail: 46 wave strips of 28 columns
  CHECK(t.tall_rpb == 131 && t.bands == 66, "x2 tail anchor: rpb %d bands %d", t.tall_rpb, t.bands);
  std::printf("%ld walks, %d failures\n", g_walks, g_fail);
  return g_fail ? 1 : 0;
}
