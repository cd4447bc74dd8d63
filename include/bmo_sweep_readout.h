/* bmo_sweep_readout.h — the through-focus and MTF read-outs of bmo.h for every configuration of a sweep, in one call each.
 *
 * bmo.h includes this header at its end: including bmo.h is enough.  BMO_ABI_VERSION is bmo.h's and unchanged.                          */
#ifndef BMO_SWEEP_READOUT_H
#define BMO_SWEEP_READOUT_H
#include "bmo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Through-focus and MTF read-out of sweeps: bmo_psf_focus_stats, bmo_psf_through_focus, bmo_psf_geo_otf and bmo_psf_otf (bmo.h
 * "Through-focus read-out", "MTF read-out") for all configurations of a bmo_trace_sweep result at once, from the rows of PSFDetector slot
 * `detector` still resident in `res`.  A loop of single calls over a thousand configurations of a thousand rows is a thousand launches that
 * do not fill the device; here the work items of all configurations run in one grid, each at its own pose, window and planes.
 *
 * Shared by the four entries, K = n_configs, M = n_planes:
 *   res, detector, n_configs : as for bmo_psf_stats_sweep.  n_configs must be the sweep's, or 1 for an ordinary result (one configuration
 *                              that owns every row); record_segments = 0 results work (the hit table is kept).
 *   origins, e1s, e2s        : [K][3], host: the detector pose of every configuration.
 *   axes                     : [K][3], host: the direction the planes of configuration c move along (bmo_psf_focus_stats's axis).
 *   offsets                  : [K][M], host: plane m of configuration c lies at origins[c] + offsets[c][m] * axes[c].
 *   displacements            : [K][M][3], host: the world vectors d_m of configuration c (bmo_psf_through_focus's displacements).
 *   xs, zs                   : [K][n], host: the sample axes of configuration c, shared by its M planes.
 *   centers                  : NULL or [K][M][2], host.      freqs : [n_freqs][2], host, shared by all configurations.
 *   outputs                  : host, configuration-major: block c has the layout of the single entry's output.
 *
 * THE CONTRACT.  Block c of every output equals, bit for bit, what the single entry returns when called on the rows of configuration c (in
 * their recorded order) with configuration c's arguments; NaN results (a row parallel to the planes, a NaN proj) included.  It holds because
 * configuration c is split exactly as a single call with its row count splits it, the rows of a split are summed in row order and the
 * splits folded in split order by the same expressions (bmo.h states them; nothing is contracted), and the value of a plane does not
 * depend on the chunk of planes it was computed with.  A configuration without rows reads what the single entry reads with n_hits = 0,
 * whatever its pose, axes and planes hold (NaN is legal there):
 *   stats : N_ROWS = 0 and NaN;   out_intensity, out_field : zeros;   otf, sums : zeros;   mtf : NaN.
 *
 * bmo_psf_focus_stats_sweep   : stats [K][M][BMO_FOCUS_STAT_N].
 * bmo_psf_through_focus_sweep : out_intensity [K][M][n*n], plane m of configuration c, element (i,j) at [((c*M + m)*n + j)*n + i];
 *                               out_field: optional, the same order as (re, im) pairs.
 * bmo_psf_geo_otf_sweep       : otf [K][M][n_freqs][2], mtf [K][M][n_freqs], sums [K][M].
 * bmo_psf_otf_sweep           : the stacks of bmo_psf_through_focus_sweep for the same arguments, transformed where they lie: only the
 *                               transfer functions leave the device (otf, mtf, sums as above), unless out_intensity [K][M][n*n] is given.
 *
 * A refused call leaves every output buffer untouched.  BMO_ERR_INVALID (checked before a device is looked for): a null pointer other than
 * centers, out_field, out_intensity and kernel_ms; n <= 0, n_planes <= 0, n_freqs <= 0; a frequency that is not finite; a slot out of range
 * or not a PSFDetector's; a wrong n_configs.  BMO_ERR_UNSUPPORTED: a GaussianBeamlet result (three rows per beamlet).  BMO_ERR_LIMIT: more
 * planes or row sums than one launch holds; for bmo_psf_geo_otf_sweep, a configuration whose partial sums would pass 4 GiB (as
 * bmo_psf_geo_otf).  BMO_ERR_INTERNAL, never a wrong answer, if the rows of a configuration are not consecutive.  kernel_ms: optional,
 * HIP-event time of the launches.
 *
 * Not here: _sweep forms of bmo_psf_geo_ee / bmo_psf_ee and of the polychromatic entries, and GaussianBeamlet results.                  */
int bmo_psf_focus_stats_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                              const double* e2s, const double* axes, const double* offsets, int32_t n_planes, double* stats,
                              double* kernel_ms);
int bmo_psf_through_focus_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                                const double* e2s, const double* displacements, int32_t n_planes, const double* xs, const double* zs,
                                int32_t n, double* out_intensity, double* out_field, double* kernel_ms);
int bmo_psf_geo_otf_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                          const double* e2s, const double* axes, const double* offsets, const double* centers, int32_t n_planes,
                          const double* freqs, int32_t n_freqs, double* otf, double* mtf, double* sums, double* kernel_ms);
int bmo_psf_otf_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                      const double* e2s, const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n,
                      const double* freqs, int32_t n_freqs, double* otf, double* mtf, double* sums, double* out_intensity, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* BMO_SWEEP_READOUT_H */
