// The sizes of csrc/sample_points.hip that its tests place their shapes around (read from this file by name, not retyped).
#pragma once

// the float64 scan of the face areas: a workgroup of SP_SCAN_THREADS threads scans one tile of SP_SCAN_THREADS x
// SP_SCAN_PER_THREAD consecutive areas of one item; the tiles' totals are scanned by one workgroup per item
constexpr int SP_SCAN_THREADS = 256;
constexpr int SP_SCAN_PER_THREAD = 8;
constexpr int SP_SCAN_TILE = SP_SCAN_THREADS * SP_SCAN_PER_THREAD;
// the coarse table of an item's cdf that a sampling workgroup keeps in LDS: at most this many float64 entries (8 KB)
constexpr int SP_TABLE = 1024;
constexpr int SP_SAMPLE_THREADS = 256;
// feature blends: below this feature dimension a loop in the sample's thread, from it on the lanes of the wavefront along the
// dimension, in groups of at least SP_FEATURE_LANE_GROUP lanes per sample.  Measured on the MI355X (profiles/sample_points_lanes_ab.jsonl,
// B = 8, F = 50 000, N = 20 000, float32, forward / forward + backward in ms): D = 8 loop 0.120 / 0.547, lanes 0.121 / 0.389; D = 16
// loop 0.192 / 0.789, lanes 0.122 / 0.435; D = 32 loop 0.422 / 1.355, lanes 0.131 / 0.469.  Below 8: not measured, the loop stays.
constexpr int SP_FEATURE_LANES_FROM = 8;
constexpr int SP_FEATURE_LANE_GROUP = 16;
