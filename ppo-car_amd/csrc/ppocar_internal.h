// ppocar_internal.h -- shared between the translation units of libppocar.so (not installed).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "ppocar.h"
#include "track_records.hpp"

struct pc_track {
    std::vector<double> walls;  // [S][4] x1,y1,x2,y2 pixels, outer segments then inner (car_env.py:653-670)
    std::vector<double> gates;  // [G][4]                      (car_env.py:671-676)
    double start_x = 0, start_y = 0, start_rot = 0;
    int n_walls() const { return (int)(walls.size() / 4); }
    int n_gates() const { return (int)(gates.size() / 4); }
};

int pc_internal_parse_track(const char* path, pc_track* t);

// ---- track_tables.cpp: the tracks compiled into the tables the env kernels read.  Host arithmetic only: no device, no HIP.
struct PairD { double x, y; };   // the device's double2 / float2, by layout (ppocar.hip asserts the sizes)
struct PairF { float x, y; };

// what dispatch needs to know of the batch's tracks, fixed once the tables are compiled.  The two layouts are the tracks'
// own: PC_OPT_ROLLOUT_FAST's nv28 switch (it can change after create) applies at dispatch.
struct TrackFacts {
    int max_G = 0, max_nV = 0, sum_nV = 0;   // reward gates, chain vertices: of the largest track; chain vertices of all tracks together
    bool tabs = true;    // every track has its gather tables (F64 handles: and the selector inside its limits and the rotation table)
    bool rden = true;    // ... its 1/den table
    bool sel = true;     // ... the selector inside its limits
    bool nv28 = true;    // ... big_track's layout: two loops of 12 walls, a padded chain of 28 vertices
    bool loops = true;   // ... two equal loops of 13 or of 9 chain vertices (big_track.json, track.json: 8 walls per loop)
};

struct TrackTables {
    std::vector<TrackHdr> hdr;        // one per track (start_collides = 0: the device computes it)
    std::vector<Seg> segs;            // the host images of the device tables (EnvParams, kernels/env_math.hpp)
    std::vector<Vtx> vtx;
    std::vector<VtxP> vtxp;           // (empty: no track of two equal chains)
    std::vector<SegD> seg64;
    std::vector<PairD> headtab;
    std::vector<PairF> dirtab;
    std::vector<PairD> dirtab64;
    std::vector<F64Dir> dirhash;      // (empty: an F32 handle, or more than 16 tracks)
    size_t rden_floats = 0;           // size of the 1/den table, which the device fills (TrackHdr::rden_off)
    std::vector<std::unordered_map<uint64_t, int>> rot_ids;   // F64, host only: per track, rotation bits -> row of the rotation table (pc_env_set_state)
    std::vector<std::vector<int>> rot_depth;                  // F64, host only: per track and row, how many turns from start_rot reach it
    TrackFacts facts;
};

// PC_OK, or PC_ERR_UNSUPPORTED with the reason in err.  R = pc_ray_count(n_nominal), dtype = PC_DTYPE_*.
int pc_internal_compile_tracks(const pc_track* const* tracks, int n_tracks, int n_nominal, int R, int dtype, TrackTables& out, std::string& err);

// How a track_id array lays the tracks over the envs: what plan_rollout's modes for mixed batches ask for.
struct TrackLayout {
    int track_block = 0;    // the largest of 256 / 128 / 64 / 32 for which every aligned block of that many envs holds ONE track (0: none)
    bool blocks32 = false;  // ... that holds for 32 (what pc_rollout needs)
    bool bal64 = false, bal32 = false;   // two tracks, interleaved, every aligned block of 64 / 32 envs split evenly between them (and N a
                                         // multiple of the block): the block's two waves de-interleave it (rollout_kernel's mode 7)
};
TrackLayout pc_internal_classify_track_ids(const uint8_t* track_id, int64_t N, int n_tracks);
