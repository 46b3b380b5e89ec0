// The row bands of FSRCNN's matrix-core mapping kernels and tails (fsrcnn.hip): how the launcher cuts `planes` planes of h rows into bands,
// and how a kernel walks its band.  Pure integer arithmetic - no HIP, no includes - so that tests/test_fsrcnn_bands_cpu.py runs the walk on
// the host over a sweep of shapes: every (plane, row) exactly once, nothing past the planned band count.
//
// Classic bands (tall_rpb == 0): every plane is cut into `bands` equal bands; band index u is band u % bands of plane u / bands: one segment.
// Tall bands (tall_rpb > 0, the default): the planes are stacked into one image of planes * h rows cut into bands of tall_rpb rows, as many
// as fill the chip's slots once; a band that straddles plane boundaries is marched as several segments, one per plane it touches.
#pragma once

#ifdef __HIPCC__
#define SS4K_FS_BANDS_HD __host__ __device__ __forceinline__
#else
#define SS4K_FS_BANDS_HD inline
#endif

namespace ss4k {
namespace fs_bands {

// per stage: the least rows of a band (every band re-does its halo rows and the pipeline fill), and slots per CU of the unit that marches a band
// on its own - a workgroup of the mapping kernels (four per CU), a wave of the tails (four waves x three workgroups per CU)
constexpr int MAPS_MIN_ROWS = 32, MAPS_SLOTS_PER_CU = 4;
constexpr int TAIL_MIN_ROWS = 16, TAIL_SLOTS_PER_CU = 4 * 3;

SS4K_FS_BANDS_HD int imin(int a, int b) { return a < b ? a : b; }

struct Plan {
  int tall_rpb;   // rows per tall band; 0: classic bands
  int bands;      // tall: bands over the stacked planes; classic: bands per plane
  int band_count(int planes) const { return tall_rpb > 0 ? bands : planes * bands; }   // the band indices that visit rows: [0, band_count)
};

// strips: column strips of the unit that marches a band; slots: how many of those units the chip holds at once.  One round of units, bands of
// at least min_rows rows.
inline Plan plan(int planes, int h, int strips, int min_rows, int slots, bool classic) {
  if (strips < 1) strips = 1;
  if (classic) {
    const int per_plane = imin((h + min_rows - 1) / min_rows, slots / (planes * strips > 1 ? planes * strips : 1));
    return {0, per_plane > 1 ? per_plane : 1};
  }
  const long rows = (long)planes * h;
  long nb = rows / min_rows < slots / strips ? rows / min_rows : slots / strips;
  if (nb < 1) nb = 1;
  const int rpb = (int)((rows + nb - 1) / nb);
  return {rpb, (int)((rows + rpb - 1) / rpb)};
}

// One band's rows, a segment at a time: rows [ylo, yhi) of `plane`.
struct Walk {
  int plane, ylo, yhi;
  int tall0, tall1;   // tall: the stacked rows of the band from the current segment on (classic: 0, 0)
  SS4K_FS_BANDS_HD bool empty() const { return ylo >= yhi; }   // (of the first segment: a band index at or past the plan's band count)
  // the following segment - the first rows of the next plane - or false: the band is done
  SS4K_FS_BANDS_HD bool next(int h) {
    tall0 += yhi - ylo;
    if (tall0 >= tall1) return false;
    plane = tall0 / h; ylo = 0; yhi = imin(h, tall1 - tall0);
    return true;
  }
};

SS4K_FS_BANDS_HD Walk first(int band, int planes, int h, int bands, int tall_rpb) {
  Walk k;
  if (tall_rpb > 0) {
    k.tall0 = band * tall_rpb; k.tall1 = imin(planes * h, k.tall0 + tall_rpb);
    k.plane = k.tall0 / h; k.ylo = k.tall0 - k.plane * h; k.yhi = imin(h, k.ylo + (k.tall1 - k.tall0));
  } else {
    const int rpb = (h + bands - 1) / bands;
    k.tall0 = k.tall1 = 0;
    k.plane = band / bands; k.ylo = (band % bands) * rpb; k.yhi = k.plane < planes ? imin(h, k.ylo + rpb) : k.ylo;
  }
  return k;
}

}  // namespace fs_bands
}  // namespace ss4k
