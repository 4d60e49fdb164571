// config.h -- kernel policy of libvfmreg_hip.so as a CALLER-OWNED object (round 6; VERDICT r5 item 7, SURVEY.md 8 B.5: "no global state
// except the last-error string").  Until round 5 the A/B switches of the test and bench tooling were process-global ints written by
// vfm_debug_set_*: two pipelines of one process with different settings raced.  Now: a vfm_config_t holds them (factory settings at
// creation), vfm_config_use() binds one to the CALLING THREAD -- thread-local, like the last-error string -- and every entry point reads
// its policy from the calling thread's binding at call time.  No binding = the immutable factory settings.
#pragma once

struct VfmConfig {
    // ---- matcher (match_api.hip, match_prep.hip, match_coarse_*.hip, match_finish.hip)
    int force_slices = 0;      // map slices of the coarse pass (0 = the launchers' rules)
    int coarse_qsets = 0;      // "coarse_variant" 0 / 1 / 2 / 4 / 5 / 10 / 12: see include/vfmreg.h, vfm_config_set
    int seed_units = 1;        // "coarse_variant" 7: no seed units
    int select_variant = 0;    // "coarse_variant" 20 / 21: general select kernel / no chunk-major rescan
    int mx6_t4 = 1;            // "coarse_variant" 30 / 31: fused fp6 half-width kernel with one (default) / two chunks per barrier
    int mx6_ns3 = 1;           // "coarse_variant" 32 / 33: ... with two / three (default) query tiles per wave at d = 384
    int prep_form = 3;         // "coarse_variant" 40, 41, 43, 44: fp6 operand preparation by prep_chunk_kernel (0) / prep_stream_kernel (1) / prep_once_kernel (3, default) /
                               // prep_once_kernel as a persistent grid, the next group's loads under a group's second pass (4)
    int finish_short = 0;      // "coarse_variant" 50 / 51: chunk-major rescan as long-lived (default) / short workgroups
    int half_noi8 = 1;         // 1 (default): callers that follow the policy (vfmreg/pipeline.py) run VFM_RECORDS_MX6_HALF_FUSED without the int8 image
                               // (VFM_PREPARE_NO_I8 + VFM_RECORDS_NO_I8); 0: with it, as before (A/B).  The library itself only stores the key.
    int rescore_block = 0;     // queries per workgroup of match_rescore_kernel: 64 (wave 0 owns them) / 256 (thread = query, lane = pair, a quarter of the
                               // workgroups, no product staging in the LDS); the same bits either way.  0 (an untouched config; "rescore_block" itself takes
                               // 64 / 256 only): by the plan -- 256 behind the half-width passes, whose lists are short, 64 elsewhere
    int rescan_rows = 1;       // "coarse_variant" 60 / 61: rescan gathers its queries from the fragment tiles / the row-major int8 scan (default)
    int mx6_tune = 0;          // (A/B) bit 0: s_setprio 1 for waves 4 - 7 of the fp6 coarse kernel; bit 1: its ring five steps deep (headline shape);
                               // bit 2: query sets past the end of the scan are multiplied as copies of tile 0 again (default: they do no matrix work)
    int match_stats = 0;       // per-query counters of a search (they cost same-address atomics)
    int i8_min_queries = 0;    // the gated family takes the int8 pass for more than this many query rows
    int prep_grid = -1;        // workgroups of prep_chunk_kernel (-1 = one per 128-row group, 0 = one per compute unit, n > 0); of the persistent
                               // prep_once_kernel: n > 0, otherwise two per compute unit of the stream
    // ---- RANSAC (ransac.hip)
    int ransac_exact_only = 0;   // 1 = every hypothesis scored in fp64 (no bounds)
    int ransac_fused = 2;        // 2 (default since round 6) = 8 launches, 1 = the 5-launch chain (slower: its one-workgroup gather), 0 = round 5's 11
    // ---- ViT (vit_plan.h resolves them, once per forward): one key per field, see include/vfmreg_debug.h
    int vit_preprocess_patch = 1, vit_xcd = 1, vit_cfg_narrow = 108, vit_cfg_wide = 108, vit_wpw = 0, vit_hot_a = 0, vit_wide_tile = 0,
        vit_lds_shape = 23, vit_att_lds_min = 1, vit_lds_min_wg = 256, vit_astat_min = 0, vit_astat_two = 1, vit_astat_nw = 0,
        vit_trace_fused = 0,   // (tools) the ONE launch of a block that gets the trace buffer: 0 the token-stationary fc1, or else the LDS-tiled fc2;
                               // 1 vit_qkv_attention_kernel; 2 the LDS-tiled proj; 3 vit_mlp_kernel
        vit_fused_mlp = 0,     // fc1 -> GELU -> fc2 of 128 tokens in one workgroup: n > 0 from n images on, -1 never, 0 vfm_vit_forward's policy
        vit_fused_qkv = 0;   // QKV + attention of an (image, head) in one workgroup: n > 0 from n images on, -1 never, 0 vfm_vit_forward's policy
    unsigned long long* vit_astat_dbg = nullptr;   // "vit_trace_buffer" (tools): device buffer of the traced launch's per-workgroup stamps
    // ---- voxel containers (voxel.hip): "voxel_small" codes
    int voxel_replay2 = 1, voxel_small = 1, voxel_trace = 0, voxel_grid_ppt = 0;
};

// the calling thread's policy (its bound vfm_config_t, or the factory settings)
const VfmConfig& vfm_cfg();
