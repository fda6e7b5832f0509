/* svihmm_debug.h -- measurement and test hooks of libsvihmm_hip.so.
 *
 * NOT the drop-in boundary (that is include/svihmm.h): nothing here replaces a reference interface.
 * bench.py uses the per-kernel HIP-event timing for the roofline object, the test suite uses
 * svihmm_set_variant to reach kernel generations the default dispatch would not pick for a shape, and
 * tools/ use both for A/B runs.  The symbols are exported by the same library so that the measured
 * binary IS the product binary; knobs that make a call's results invalid (skipped launches, knocked-out loads /
 * stores) are compiled only with -DSVIHMM_MEASURE (make -C pysvihmm_amd/csrc measure ->
 * build_exp/libsvihmm_measure.so, never shipped): no code of a product build leaves anything uncomputed.
 *
 * Versioning: SVIHMM_ABI_VERSION / svihmm_abi_version() cover include/svihmm.h ONLY (the symbols a caller of the
 * product binds; 3 since the hooks below left that header in round 5).  This header is not a stable interface: it
 * changes with the library build (round 6 added svihmm_svi_recoveries and the codes SVI_LOOP = 2 / 3,
 * PIPELINE = 3 / 5, WIDE_SWEEPS = 3), and its only users are the repository's own tests, bench.py and tools/,
 * which travel with the library.
 */
#ifndef SVIHMM_DEBUG_H
#define SVIHMM_DEBUG_H

#include "svihmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement ------------------------------------------------------------------ */
/* When enabled, every kernel launched by the handle is bracketed by HIP events on
 * the handle's stream; svihmm_profile_read returns accumulated milliseconds and
 * launch counts per kernel slot since the last reset. */
#define SVIHMM_NKERN 12
/* on = 0: off; 1: every slot; SVIHMM_PROF_SLOTS | (1 << slot) | ...: those slots only (an event
 * pair between two dependent kernels costs a few microseconds of dispatch -- measured 0.055 ms on
 * the 3.15 ms bench step with all slots -- so a timed region that wants one kernel's duration
 * brackets only that kernel). */
#define SVIHMM_PROF_SLOTS 0x40000000
int svihmm_profile_enable(svihmm_ctx* h, int32_t on);
int svihmm_profile_reset(svihmm_ctx* h);
int svihmm_profile_read(svihmm_ctx* h, double ms_out[SVIHMM_NKERN],
                        int64_t count_out[SVIHMM_NKERN]);
const char* svihmm_kernel_name(int32_t slot);
/* The kernel function the slot's LAST launch dispatched, as rocprofv3 prints it (e.g.
 * "k_stats_mfma4<5, 2, 2, 3, true, false, double, double, 3, 1>"; "" when unknown): bench.py checks it against
 * the kernel name in the committed profile before it quotes that profile's duration. */
const char* svihmm_last_kernel_name(svihmm_ctx* h, int32_t slot);
/* ---- kernel-selection knobs (svihmm_set_variant) ------------------------------------------ */
/* svihmm_set_variant(h, which, value) selects a kernel generation for A/B measurement and for tests: `which` is one
 * of the slots below (which < SVIHMM_NVARIANT), `value` one of the slot's codes; 0 is always the default dispatch.
 * This table is the only place where the slots and codes are written down: the host code under pysvihmm_amd/csrc
 * reads the knobs by these names, pysvihmm_amd/_lib.py's VARIANT mirrors the slot names (tests/test_variant_table.py).
 * The numbers are fixed: tools/ and the committed profiles refer to them.  Some slots carry two unrelated switches
 * (5, 7, 9, 10, 12, 13); their entries say so. */
#define SVIHMM_NVARIANT 24      /* size of the handle's knob array: slots 18 .. 23 are accepted and read by nothing */
enum {
  /* 0: the resident SVI loop's dependency mechanism (0: device-side counters where kernels of two streams run side
   *    by side, else stream events) -- and one measurement code */
  SVIHMM_VAR_SVI_LOOP = 0,
  /* 1: statistics GEMM generation (0: the pipelined MFMA kernels where they fit) */
  SVIHMM_VAR_STATS = 1,
  /* 2: sweep implementation (0: chosen per batch, pick_fb) */
  SVIHMM_VAR_FB = 2,
  /* 3: LDS-staged emission GEMM k_emission_mfma: row tiles per wave.  The value is a COUNT, 2 (default) or 4; any
   *    other value runs 2 */
  SVIHMM_VAR_EMISSION_MT = 3,
  /* 4: E-step launch structure (0: sweeps + statistics of minibatch-sized K = 64 batches in one fused launch where
   *    that is ahead, else one launch after the other; 4: as 0).  Whatever this slot says, the fused launch needs STATS,
   *    SWEEP_FAMILY, STATS_CHUNKS, STATS_TILING and WIDE_POSTERIOR at 0 and FB at 0 or 3 */
  SVIHMM_VAR_PIPELINE = 4,
  /* 5: emission kernel choice.  Two switches: codes 1 / 2 / 5 / 6 / 7 shape the fp64 orbit-schedule kernels (K <= 64,
   *    D % 8 == 0, 8 <= D <= 40; 6 / 7 keep the row-tile kernel's generic staging and epilogue in every workgroup),
   *    codes 3 / 4 / 8 the fp32 mode's bf16 x 3 kernels.  The emission tiles inside the fused E-step launch
   *    (PIPELINE 3 / 5) need this slot at 0 */
  SVIHMM_VAR_EMISSION_ORBIT = 5,
  /* 6: blocked scan for one long window (B = 1, Lm >= 2048, K <= 256) and blocked backward sampling of the FFBS
   *    entry points (chains / windows of at least 1024 rows) */
  SVIHMM_VAR_CHAIN = 6,
  /* 7: scaled sweeps' kernel family.  Two switches: codes 1 / 2 choose the state tiles per wave of wide models
   *    (K > 128; 2 also keeps every K <= 64 batch on the MFMA tile kernels), codes 3 / 4 the minibatch kernel that
   *    gives one window to one wave -- and one measurement code */
  SVIHMM_VAR_SWEEP_FAMILY = 7,
  /* 8: row chunks of the statistics GEMM.  The value is a COUNT, not a code: 0 automatic (stats_plan), n > 0 asks for
   *    n chunks (rounded to whole row blocks) */
  SVIHMM_VAR_STATS_CHUNKS = 8,
  /* 9: two switches: automatic centring of the resident observations at upload (code 1), and how a synchronous
   *    E-step call's window starts reach the device (code 2) */
  SVIHMM_VAR_CENTRING = 9,
  /* 10: statistics GEMM tiling (code 1) and, a second switch, the fp32 mode's pipe (codes 2 / 3; they also steer the
   *    mode's emission kernels for 32 < D <= 64 and wide models, which enter the fp32 format only together with
   *    their statistics kernel) */
  SVIHMM_VAR_STATS_TILING = 10,
  /* 11: svihmm_allreduce_packed forms the sum in caller coordinates also at one rank */
  SVIHMM_VAR_ALLREDUCE_COORDS = 11,
  /* 12: barrier-free statistics GEMM with three LDS buffers (code 1), and how that kernel's staging threads address
   *    obs / ah / bh (code 2) */
  SVIHMM_VAR_STATS_LDS3 = 12,
  /* 13: two switches: wide models' sweeps with 32 windows per workgroup (code 1), and the NIW -> theta builder
   *    for 16 < D <= 32 (codes 2 / 3) */
  SVIHMM_VAR_WIDE_SWEEPS = 13,
  /* 14: wide models' transition statistic in 128 x 64 blocks */
  SVIHMM_VAR_WIDE_TRAN_BLOCK = 14,
  /* 15: wide models' statistics GEMM forms q = ah bh scale itself */
  SVIHMM_VAR_WIDE_POSTERIOR = 15,
  /* 16: the register-resident minibatch sweep (k_wave_linr, the sweep workgroups of k_sweep_stats) re-normalises its
   *    vector every fourth step where the transition expectations lie inside a float's range */
  SVIHMM_VAR_RENORM4 = 16,
  /* 17: message layout of the tiled fp64 epoch at K = 64 (0: Eh / ah / bh step-major inside each 16-window group,
   *    csrc/kernels_msg_layout.h) */
  SVIHMM_VAR_MSG_LAYOUT = 17
};
/* The codes, per slot.  A code that is not listed behaves as 0 unless the slot's entry above says otherwise. */
enum {
  /* SVI_LOOP */
  SVIHMM_SVI_LOOP_EVENTS = 1,            /* stream events (the choreography of rounds 2-4) */
  SVIHMM_SVI_LOOP_LOSE_CONCURRENCY = 2,  /* debug: counters, and the loop behaves as if the device stopped running kernels
                                            concurrently at iteration 3 -- exercises the mid-loop switch to stream events */
  SVIHMM_SVI_LOOP_STUCK_GATE = 3,        /* debug: counters, one gate of iteration 3 waits for a count that never comes with
                                            a 2 ms bound -- exercises the bounded-wait recovery */
  SVIHMM_SVI_LOOP_NO_ELBO = 9,           /* MEASURE build only: the loop's ELBO kernels are not launched, so the ELBO trace
                                            (svihmm_svi_read_elbo) is not computed; the iterations themselves are valid.
                                            A product build accepts the value and never reads it: as 0 */
  /* STATS */
  SVIHMM_STATS_DBUF = 2,                 /* the double-buffered MFMA kernels */
  SVIHMM_STATS_PIPELINED = 3,            /* the pipelined MFMA kernels, which the statistics launch takes for every value but
                                            2; unlike 0, any non-zero value also keeps the fused E-step launch and the fp32
                                            mode's bf16 statistics kernels off (the two-stream pipeline accepts 0 and 3) */
  /* FB: also what pick_fb returns for a batch */
  SVIHMM_FB_WAVE = 1,                    /* wave-per-window, log domain */
  SVIHMM_FB_LOG_MFMA = 2,                /* log-domain MFMA (K <= 64; beyond: as 1) */
  SVIHMM_FB_SCALED = 3,                  /* scaled linear-domain MFMA */
  /* EMISSION_MT (a count; one value has a second meaning) */
  SVIHMM_EMISSION_MT_NT4 = 1,            /* two row tiles, and wide models keep four state tiles per wave instead of eight */
  /* PIPELINE */
  SVIHMM_PIPELINE_UNFUSED = 1,           /* never the fused launch, never two streams */
  SVIHMM_PIPELINE_TWO_STREAM = 2,        /* the two-stream pipeline of round 2 (B >= 32) */
  SVIHMM_PIPELINE_FUSED_ALL = 3,         /* tests: the fused launch for every batch it can take, whatever its size or
                                            precision mode, WITH the emission tiles computed inside it where the batch's
                                            emission kernel is the 16-row fp64 one (D % 8 == 0, D <= 32) */
  SVIHMM_PIPELINE_FUSED_EMISSION = 5,    /* as 0 plus the emission tiles inside the launch -- measured, not ahead:
                                            tu_fused.hip, sweep_emission_ok */
  SVIHMM_PIPELINE_F32_OWN = 6,           /* as 0, but the fp32 mode keeps float messages + its bf16 statistics kernel for
                                            minibatch-sized batches instead of the fused launch on fp64 messages behind
                                            float emission rows */
  /* EMISSION_ORBIT */
  SVIHMM_EMISSION_ORBIT_OFF = 1,         /* the LDS-staged GEMM k_emission_mfma instead of the orbit-schedule kernels */
  SVIHMM_EMISSION_ORBIT_128 = 2,         /* always k_emission_orbit with 128-row workgroups */
  SVIHMM_EMISSION_ORBIT_F64 = 3,         /* fp32 mode: the fp64 feature GEMMs instead of the bf16 x 3 kernels (the batch
                                            then never enters the wide models' fp32 format) */
  SVIHMM_EMISSION_ORBIT_BF16_SMALL = 4,  /* fp32 mode, K <= 64, D <= 32: the bf16 x 3 kernel also below 8192 rows */
  SVIHMM_EMISSION_ORBIT_64 = 5,          /* minibatches: the 64-row k_emission_orbit of round 3 instead of the 16-row
                                            k_emission_orbit_ks */
  SVIHMM_EMISSION_ORBIT_GENERIC_EDGES = 6,       /* default dispatch, but the row-tile kernel k_emission_orbit runs its
                                                    generic staging and epilogue in every workgroup instead of the lean
                                                    ones in workgroups wholly inside the batch (K = Kp, fp64 storage;
                                                    csrc/kernels_emission.h) -- same results bit for bit */
  SVIHMM_EMISSION_ORBIT_128_GENERIC_EDGES = 7,   /* codes 2 and 6 together (tests: batches below one workgroup per CU) */
  SVIHMM_EMISSION_ORBIT_BF16_128 = 8,   /* fp32 mode minibatches: k_emission_bf16x3<1>, one group of four waves on 128
                                            rows, instead of k_emission_bf16x3h */
  /* CHAIN */
  SVIHMM_CHAIN_OFF = 1,
  /* SWEEP_FAMILY */
  SVIHMM_SWEEP_FAMILY_ONE_TILE = 1,      /* K > 128: one state tile per wave for every K */
  SVIHMM_SWEEP_FAMILY_TILES = 2,         /* K > 128: two state tiles per wave for every K; K <= 64: the MFMA tile kernels
                                            also for batches small enough for the wave-per-window ones */
  SVIHMM_SWEEP_FAMILY_WAVE_LIN = 3,      /* minibatches: the LDS-broadcast one-wave k_wave_lin instead of the
                                            register-resident k_wave_linr (fp64) / the four-wave k_wave_lin4 (fp32 mode) */
  SVIHMM_SWEEP_FAMILY_WAVE_LIN4 = 4,     /* fp32 mode minibatches: the four-wave k_wave_lin4 instead of k_wave_linr with
                                            fp64 arithmetic on float storage */
  SVIHMM_SWEEP_FAMILY_SKIP = 9,          /* MEASURE build only, results INVALID: the scaled sweeps are skipped, the
                                            statistics read stale messages (tools/r4_overlap_probe.py) */
  /* CENTRING */
  SVIHMM_CENTRING_OFF = 1,               /* no automatic centring: c = 0 */
  SVIHMM_CENTRING_PULL_STARTS = 2,       /* centring as 0; a synchronous E-step's window starts go through the copy kernel
                                            (k_pull) instead of the mapped slot the emission kernel reads itself */
  /* STATS_TILING */
  SVIHMM_STATS_TILING_FIVE = 1,          /* five feature tiles per wave for every shape */
  SVIHMM_STATS_TILING_F32_MFMA = 2,      /* fp32 mode: the fp32-input MFMA kernel instead of the three-term bf16 one */
  SVIHMM_STATS_TILING_BF16_SMALL = 3,    /* fp32 mode: the bf16 kernels also below their batch-size floor of 32 768 rows */
  /* ALLREDUCE_COORDS */
  SVIHMM_ALLREDUCE_COORDS_ON = 1,        /* the multi-rank path's coordinate round trip, exercised on a single GPU */
  /* STATS_LDS3 */
  SVIHMM_STATS_LDS3_OFF = 1,             /* the double-buffered kernel */
  SVIHMM_STATS_LDS3_FLAT = 2,            /* the three-buffer kernel, but its staging loads stay flat loads from clamped
                                            addresses behind value selects instead of buffer loads with 32-bit lane
                                            offsets (csrc/kernels_stats.h, SG) -- same results bit for bit */
  /* WIDE_SWEEPS */
  SVIHMM_WIDE_SWEEPS_16 = 1,             /* 16 windows per workgroup */
  SVIHMM_WIDE_SWEEPS_THETA_OLD = 2,      /* NIW -> theta for 16 < D <= 32 by the builder that leaves half the wave idle
                                            (rounds 2-5) instead of k_niw_to_theta_wave32s -- same results bit for bit */
  SVIHMM_WIDE_SWEEPS_THETA_OWN_STEP = 3, /* the split builder, but the resident loop's global step stays a launch of its
                                            own (k_svi_global_step, not merged into k_svi_step_theta32s) */
  /* WIDE_TRAN_BLOCK */
  SVIHMM_WIDE_TRAN_BLOCK_64 = 1,         /* 64 x 64 blocks */
  /* WIDE_POSTERIOR */
  SVIHMM_WIDE_POSTERIOR_PASS = 1,        /* K > 64: separate posterior pass */
  SVIHMM_WIDE_POSTERIOR_PASS_ALL = 2,    /* a separate pass for every K -- valid results, slower */
  /* RENORM4 */
  SVIHMM_RENORM4_OFF = 1,                /* every step; same results bit for bit */
  /* MSG_LAYOUT */
  SVIHMM_MSG_LAYOUT_ROW_MAJOR = 1        /* row-major as on every other path -- same results bit for bit */
};
/* Codes that make a call's RESULTS invalid exist only in a -DSVIHMM_MEASURE build of the library (make measure):
 * that is SWEEP_FAMILY = SVIHMM_SWEEP_FAMILY_SKIP, which a product build rejects with an error.  The other code
 * read only under -DSVIHMM_MEASURE, SVI_LOOP = SVIHMM_SVI_LOOP_NO_ELBO, leaves results valid and only the ELBO trace
 * out; a product build accepts it and ignores it. */
int svihmm_set_variant(svihmm_ctx* h, int32_t which, int32_t value);
/* How often the current device-resident SVI loop left its device-side counters for stream events mid-way
 * (a gate's bounded wait ran out and the lost iterations were replayed, or the debug codes SVI_LOOP = 2 / 3). */
int svihmm_svi_recoveries(svihmm_ctx* h, int32_t* out);

/* ---- diagnostics ------------------------------------------------------------------- */
/* One v_mfma_f64_16x16x4_f64 on A[16,4] x B[4,16] -> C[16,16] (operand-layout check). */
int svihmm_selftest_mfma(svihmm_ctx* h, const double* A16x4, const double* B4x16,
                         double* C16x16);

#ifdef __cplusplus
}
#endif
#endif /* SVIHMM_DEBUG_H */
