// rm_rows.h -- the frame rows of one launch (plain integer logic, no HIP).
#pragma once

namespace rm {

// The frame rows one launch renders: y with (y mod cycle) - offset in [0, run)
// (round-robin bands: run = band, cycle = band * nshards, offset = band * shard).
struct RowPart {
    int cycle, offset, run;
};
// validated row part of round-robin bands, or of an explicit cyclic part
inline bool band_part(int band, int nshards, int shard, RowPart &p) {
    if (band <= 0 || nshards <= 0 || shard < 0 || shard >= nshards || (long long)band * nshards > 0x7fffffffLL) return false;
    p = RowPart{band * nshards, band * shard, band};
    return true;
}
inline bool cycle_part(int cycle, int offset, int run, RowPart &p) {
    if (cycle <= 0 || offset < 0 || run <= 0 || (long long)offset + run > cycle) return false;
    p = RowPart{cycle, offset, run};
    return true;
}
// FrameConst.tile_run (rm_device.h; shard_row_of_wave, rm_render_direct.h): how packed rows row0 + [jb, jb + wave_h),
// jb a multiple of wave_h, map to frame rows.  1: the part is every row of the frame (cycle = run, offset 0:
// y = j); 2: they lie in one run (wave_h divides the run length and row0), and the launch divides by a magic
// multiplier (has_magic); 0: neither, each lane finds its own row
inline int wave_row_mode(const RowPart &p, int row0, int wave_h, bool has_magic) {
    if (p.cycle == p.run && p.offset == 0) return 1;
    return has_magic && p.run % wave_h == 0 && row0 % wave_h == 0 ? 2 : 0;
}
inline int rows_of_part(int H, const RowPart &p) {
    const long long full = H / p.cycle, rest = H - full * p.cycle;
    long long tail = rest - p.offset;
    tail = tail < 0 ? 0 : tail > p.run ? p.run : tail;
    return (int)(full * p.run + tail);
}

}  // namespace rm
