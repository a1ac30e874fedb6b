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
inline int rows_of_part(int H, const RowPart &p) {
    const long long full = H / p.cycle, rest = H - full * p.cycle;
    long long tail = rest - p.offset;
    tail = tail < 0 ? 0 : tail > p.run ? p.run : tail;
    return (int)(full * p.run + tail);
}

}  // namespace rm
