/*
 * mdhip.h -- C ABI of libmdhip.so: the MI355X (gfx950) force + velocity-Verlet + thermostat
 * path behind MolecularDynamics.jl's Parameters / SimulationState / Potential / evaluate /
 * run_simulation! surface.
 *
 * Every entry point is extern "C", takes plain integers, doubles and pointers, returns an
 * int status (0 = ok, non-zero = error; text via md_last_error) and never lets a C++
 * exception cross the boundary.  Host arrays are borrowed for the duration of one call;
 * device memory is owned by the handle.  A handle is bound to one GPU and is not
 * re-entrant.  Citations are  file:line  into the reference (edwinb-ai/MolecularDynamics.jl
 * v0.7).
 *
 * Host array layout: column-major d x N, i.e. particle i's component c at a[i*d + c]
 * (a Julia Matrix{Float64}(d, N); the Julia wrapper packs its Vector{MVector{d}} into one).
 * Particle indices are 0-based at this boundary.
 */
#ifndef MDHIP_H
#define MDHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_ctx md_ctx;

/* Potential kinds for md_set_potential.  params layout per kind:
 *   MD_POT_LJ            {epsilon, sigma, r_cut}   src/potentials.jl:41-64,66-77,160-164
 *                         (sigma is unused by the pair term, as in the reference: the pair
 *                          sigma comes from the two diameters)
 *   MD_POT_PSEUDOHS      {lambda}                  src/potentials.jl:1-29
 *   MD_POT_POLYDISPERSE  {r_cut, non_additivity}   README.md:89-145 (user potential example)
 *   MD_POT_LJ_MODIFIED   {epsilon, sigma, r_cut, mode, r_on}  the reference's shifted (mode 0,
 *                         src/potentials.jl:79-90), force-shifted (1, :92-103) and XPLOR-switched (2,
 *                         :195-238) Lennard-Jones: dead code there (evaluate never dispatches to them),
 *                         reachable here.  V_cut, F_cut follow the constructor (:52-64).
 *   MD_POT_CUSTOM        set through md_set_potential_source (hiprtc)                      */
enum { MD_POT_LJ = 0, MD_POT_PSEUDOHS = 1, MD_POT_POLYDISPERSE = 2, MD_POT_LJ_MODIFIED = 3, MD_POT_CUSTOM = 100 };

/* Ensemble kinds for md_run: src/types.jl:34-51, src/integrate.jl:40-53 */
enum { MD_NVE = 0, MD_NVT = 1 };

/* Replaces CellListMap.ParticleSystem(xpositions, unitcell, cutoff, ...) +
 * SimulationState's device-side half: src/initialization.jl:100-107, src/types.jl:15-32.
 * box is the d x d unit cell, column-major, COLUMNS = lattice vectors (Julia's Matrix as
 * src/initialization.jl:7-18 builds it).  A diagonal matrix is an orthorhombic cell (the fast
 * paths); any other non-singular matrix is a general (triclinic) cell: positions wrap as
 * wrap_to_box does (src/boundary.jl:7-17: frac = U^-1 x, image += floor.(frac),
 * x = U (frac - floor.(frac))), periodic images are lattice-vector translations, and the linked
 * cells are cut in fractional coordinates -- every pair of opposite cell faces must be at least
 * 3 list radii apart (md_create / md_set_skin fail otherwise).  General cells are single-handle:
 * md_create_domain refuses them.  list_cutoff is CellListMap's cutoff (independent
 * of the potential's own r_cut).  device_id < 0 means "current device".               */
int md_create(int dim, int64_t n_particles, const double *box, double list_cutoff, int device_id, md_ctx **out);
int md_destroy(md_ctx *ctx);

/* Last error text for a handle; with ctx == NULL, the last error of a failed md_create. */
const char *md_last_error(md_ctx *ctx);

/* Replaces compile-time dispatch of evaluate(pot::P, r, s1, s2): src/pairwise.jl:28-31,
 * src/types.jl:1-6. */
int md_set_potential(md_ctx *ctx, int kind, const double *params, int nparams);

/* User-defined potential compiled at run time (hiprtc).  hip_src must define
 *   __device__ void <entry_name>(double r, double sigma1, double sigma2,
 *                                const double* params, double* u, double* f);
 * returning the pair energy u and f = -dU/dr exactly like the reference's evaluate
 * contract (README.md:86-88,116-117). */
int md_set_potential_source(md_ctx *ctx, const char *hip_src, const char *entry_name, const double *params,
                            int nparams);

/* Verlet-list skin.  skin = 0 rebuilds the linked cells every step exactly as
 * CellListMap.map_pairwise! does (src/simulation.jl:100-104); skin > 0 reuses a neighbour
 * list built with cutoff+skin until some particle has moved skin/2 -- the accepted pair set
 * of every step is unchanged (pairs are still filtered by d^2 <= list_cutoff^2).  Default: 0.6
 * (0.4 for a slab-decomposition handle), clipped to what the box allows.                  */
int md_set_skin(md_ctx *ctx, double skin);

/* Dynamic pruning of the rows: every few steps the rows the force kernel walks are refreshed from
 * the Verlet rows, keeping the entries within list_cutoff + inner_skin at that moment.  Results are
 * unchanged (only sure misses are dropped, order kept); inner_skin = 0 turns it off.  Default 0.16. */
int md_set_inner_skin(md_ctx *ctx, double inner_skin);

/* State transfer; any pointer may be NULL (= leave that array as it is on the device).
 * x, v, f: d x N doubles; images: d x N int32; diameters: N doubles.
 * Mirrors the fields of SimulationState / EnergyAndForces: src/types.jl:15-32,53-57.
 * Forces persist across md_run calls and start at whatever was uploaded. */
int md_upload(md_ctx *ctx, const double *x, const double *v, const double *f, const int32_t *images,
              const double *diameters);
int md_download(md_ctx *ctx, double *x, double *v, double *f, int32_t *images);

/* reset_output! + CellListMap.map_pairwise!(energy_and_forces!, system):
 * src/pairwise.jl:6-15,26-39; src/simulation.jl:99-104.  Leaves forces on the device,
 * returns the potential energy U and the virial W = sum_pairs f_ij . r_ij.              */
int md_compute_forces(md_ctx *ctx, double *energy, double *virial);

/* The accepted pair set of the current positions: every unordered pair {i,j} with
 * d^2 <= list_cutoff^2, as (min,max) 0-based int32 pairs, unsorted.  count receives the
 * number found; at most cap pairs are written.  (CellListMap's pair enumeration, exposed
 * for the bit-exact neighbour-index parity check.)                                       */
int md_neighbor_pairs(md_ctx *ctx, int32_t *pairs, int64_t cap, int64_t *count);

/* The step loop of run_simulation!: src/simulation.jl:88-108 --
 *   integrate_half! (src/integrate.jl:8-21, wrap src/boundary.jl:7-17) -> reset_output! ->
 *   map_pairwise! -> integrate_second_half! (src/integrate.jl:28-38) -> ensemble_step!
 *   (src/integrate.jl:40-53; bussi! src/thermostat.jl:20-48).
 * Runs nsteps steps device-resident.  For MD_NVT, ktemp[s], r1[s], r2[s] (s = 0..nsteps-1)
 * are the target temperature ens.ktemp(step+1) and the two random draws of bussi! for step
 * s (r1 = randn, r2 = sum_noises(nf-1), src/thermostat.jl:1-18,32-33): the RNG stays on the
 * host.  nf is SimulationState.nf = d*(N-1) (src/initialization.jl:124).
 * If uwk != NULL it receives {U, W, K} of the LAST step (potential energy, virial, kinetic
 * energy after the thermostat) -- what the thermo line of src/simulation.jl:118-136 needs.
 * Stated deviation: the reference rebuilds its cells every step and keeps stepping (and printing NaN / garbage) when a
 * system blows up; md_run follows its Verlet rows and returns an error when a particle moves more than half the list skin
 * in ONE step three times over at the same step (no list can follow that).  Non-finite coordinates that do not trip the
 * displacement test are carried along as the reference carries them.                                                  */
int md_run(md_ctx *ctx, int64_t nsteps, double dt, int ensemble, double tau, double nf, const double *ktemp,
           const double *r1, const double *r2, double *uwk);

/* fire_minimize!: src/minimize.jl:31-135 -- FIRE relaxation on the same force path, device resident (the whole
 * scalar state -- dt, alpha, counters, convergence -- lives on the device; the host only waits every 32 steps).
 * Positions, images and forces of the handle are updated; its velocities are left as they were (FIRE's own
 * velocities are internal and start at zero, :57).  Keyword defaults of the reference: max_steps 10000,
 * tol 1e-6, dt_initial 0.01, dt_max 0.1, alpha0 0.1, f_inc 1.2, f_dec 0.2, Nmin 5.  *steps = force evaluations
 * consumed by the loop (the converging one included); *energy, *f_rms = F_norm/sqrt(d(N-1)) of the last force
 * evaluation (after max_steps without convergence that is the closing evaluation of :126-129).            */
int md_fire_minimize(md_ctx *ctx, int64_t max_steps, double tol, double dt_initial, double dt_max, double alpha0,
                     double f_inc, double f_dec, int nmin, int64_t *steps, int *converged, double *energy,
                     double *f_rms);

/* The Brownian step loop (src/simulation.jl:181-308 + integrate_brownian! src/integrate.jl:66-82; broken in the
 * reference; restated here):  per step  forces at x ;  x += f*dt/kT + sqrt(2 dt)*noise ,
 * noise_c = (2u-1)*sqrt(3).  The reference draws u from one host RNG shared by its threads; here u comes from a
 * counter-based stream -- Philox4x32-10, key = seed, counter = (0-based particle index, first_step + s) --
 * so a trajectory depends on neither thread layout nor particle order and a host can reproduce it.
 * out = {U, W of the last step's force evaluation, sum of the virial over the steps with
 * (first_step + s) % virial_every == 0 (the reference samples every 10th step), number of such steps}.
 * nsteps == 0 evaluates nothing: out = {0, 0, 0, 0} and the state is left as it is.                         */
int md_run_brownian(md_ctx *ctx, int64_t nsteps, double dt, double ktemp, uint64_t seed, int64_t first_step,
                    int64_t virial_every, double *out /* [4] */);

/* Frame export at the trajectory cadence (src/simulation.jl:139-171: the dump holds positions and image counters).
 * md_snapshot_begin gathers both in original-particle order (positions wrapped exactly as md_download wraps them) and
 * starts the device-to-host copy into pinned memory on a copy stream of the library; it does NOT wait.  The caller may
 * enqueue the next segment (md_run ...) at once: the copy overlaps it.  md_snapshot_end waits for the copy and fills the
 * caller's d x N column-major arrays (either may be NULL).  One frame in flight per handle. */
int md_snapshot_begin(md_ctx *ctx);
int md_snapshot_end(md_ctx *ctx, double *x, int32_t *images);

/* Radial distribution function, sampled on the device (new relative to the reference, whose users histogram dumped
 * trajectories on the host).  md_rdf_setup allocates the sampler, uploads the squared bin edges
 * e2[k] = (k*delta)^2, delta = r_max / nbins, and zeroes the histogram; calling it again starts over.  Needs
 * 1 <= nbins <= 8192, r_max > 0 and every face distance >= 3*r_max (the rule md_create applies to the list cutoff);
 * a slab-decomposition handle is refused.  md_rdf_sample adds one sample of the current positions -- wrapped exactly
 * as md_download returns them -- to the histogram, on the handle's stream, without waiting; it changes nothing the
 * handle computes afterwards.  The unordered pair {a, b}, a < b, with del = (x_b + t) - x_a (t = the periodic
 * translation bringing b next to a) and d2 = (del0*del0 + del1*del1) + del2*del2, goes into bin k iff
 * e2[k] <= d2 < e2[k+1].  md_rdf_read waits and returns counts[nbins], summed over the samples since setup or the last
 * md_rdf_reset, and their number; md_rdf_reset zeroes both and keeps the setup.                                   */
int md_rdf_setup(md_ctx *ctx, double r_max, int nbins);
int md_rdf_sample(md_ctx *ctx);
int md_rdf_read(md_ctx *ctx, int64_t *counts, int64_t *nsamples);
int md_rdf_reset(md_ctx *ctx);

/* Self dynamics, sampled on the device (new relative to the reference, whose users compute them on the host from the
 * log-time LAMMPS frames with unwrapped columns).  A frame is exactly what md_download returns at that moment: the
 * wrapped x and the image counts n, in particle-id order, written by the same gather into buffers the sampler owns.
 * For one origin frame t0 and one current frame t, particle i contributes
 *   dn_c  = (double)n_c(t) - (double)n_c(t0)                                     (exact)
 *   del_c = (x_c(t) - x_c(t0)) + ((U_c0*dn_0 + U_c1*dn_1) + U_c2*dn_2)         (2-D: no third term)
 *   d2    = (del_0*del_0 + del_1*del_1) + del_2*del_2,   d4 = d2*d2
 *   s(q)  = sum over the axes c = 0..d-1, in order, of cos(q*del_c)            (for each of the nq wavenumbers)
 * with every operation rounded on its own (no fma).  U_cr is the unit cell's row c, column r.  For a diagonal cell the
 * off-diagonal products are zeros, so del_c is x_c(t) - x_c(t0) + L_c*dn_c bit for bit (d2 sees at most the sign of a
 * zero).  The wrapped coordinates are differenced before the lattice translation is added, so no precision is lost to
 * large unwrapped coordinates; the reference's p + boxmat*img (a BLAS product) has no pinned order and is not restated.
 * The van Hove histogram counts d2 in bin k iff e2[k] <= d2 < e2[k+1], e2[k] = (k*delta)*(k*delta), delta =
 * r_max/nbins, a host table built as md_rdf_setup builds it; d2 >= e2[nbins] is not counted.  Counts are integers.
 * The sums {sum d2, sum d4, sum s(q_0), ..., sum s(q_nq-1)} are fp64, reduced over particle ids in a tree fixed by N
 * (wave, then block partials in block order, then one block) without floating-point atomics: the same pair of frames
 * gives the same bits on any handle, whatever its list history.  Each sample's totals are added into its row's running
 * sums in stream order.
 *
 * md_dyn_setup allocates nslots origin slots (nslots*N*d*12 bytes) and nrows rows, zeroed; calling it again starts over.
 * Needs 1 <= nslots <= 64, nrows >= 1, 0 <= nq <= 16 finite q, 0 <= nbins <= 8192 and, when nbins > 0, a finite
 * r_max > 0.  md_dyn_origin stores the current frame in `slot`; md_dyn_sample exports the current frame once and adds
 * `count` samples, frame vs slots[i] into rows[i]; neither waits, and neither changes anything the handle computes
 * afterwards.  md_dyn_read waits and returns nsamples[nrows], sums[nrows*(2+nq)] and, if hist is not NULL,
 * hist[nrows*nbins]; md_dyn_reset zeroes the rows and keeps the setup and the stored origins.  A slab-decomposition
 * handle, a slot or row out of range, an empty slot and any call before md_dyn_setup are refused.               */
int md_dyn_setup(md_ctx *ctx, int nslots, int nrows, const double *q, int nq, double r_max, int nbins);
int md_dyn_origin(md_ctx *ctx, int slot);
int md_dyn_sample(md_ctx *ctx, const int32_t *slots, const int32_t *rows, int count);
int md_dyn_read(md_ctx *ctx, int64_t *nsamples, double *sums, int64_t *hist);
int md_dyn_reset(md_ctx *ctx);

/* Density modes, the static structure factor S(q) and the coherent intermediate scattering function F(q, t), sampled on
 * the device (new relative to the reference, whose users compute them on the host from dumped frames).  A wave vector is
 * an integer tuple n (d components), q_n = 2*pi*U^-T n, so q_n.x = 2*pi*n.f with f = U^-1 x the fractional coordinate:
 * the phase does not depend on the image counts, and the sampler reads only the wrapped coordinates of a frame -- what
 * md_download returns at that moment, in particle-id order, written by the same gather into a buffer the sampler owns.
 * Sign convention: rho(q) = sum over particles of exp(+i q.x).  Per particle and vector
 *   f_c = x_c / L_c (diagonal cell)   or   f_c = (Uinv_c0*x_0 + Uinv_c1*x_1) + Uinv_c2*x_2 (general cell)
 *   t   = (n_0*f_0 + n_1*f_1) + n_2*f_2,  r = t - rint(t) (exact)                  (2-D: no third term)
 * and the particle adds (cos 2*pi*r, sin 2*pi*r) to (Re rho, Im rho); everything in fp64, every operation of t rounded on
 * its own.  The sum over particles is a tree fixed by N alone, without floating-point atomics, so rho is a function of
 * the frame only (the same bits on any handle, whatever its skin, list history or cell order), and per component
 *   |rho - rho_true| <= N * (32*kappa*|n|_1 + 128) * 2^-53,   kappa = || |U^-1| |U| ||_inf  (1 for a diagonal cell).
 * Accumulators, fp64, no fma, added in stream order: s2[v] += Re*Re + Im*Im (static), and for a sample of the current
 * frame against origin slot s into row k, corr[k][v] += Re_now*Re_s + Im_now*Im_s.
 *
 * md_sq_setup takes nvec vectors (n[v*d + c], 1 <= nvec <= 16384, |n_c| <= 32767, n != 0), 0 <= nslots <= 64 origin
 * slots of 2*nvec doubles and nrows >= 0 correlation rows, all zeroed; calling it again starts over.  md_sq_sample
 * evaluates rho of the current frame once, then, in this order: adds it to the static accumulator if add_static != 0,
 * adds the `count` correlations (frame vs slots[i] into rows[i]), and stores rho in origin_slot unless that is -1.  It
 * does not wait and changes nothing the handle computes afterwards.  md_sq_rho waits and returns rho of the last sampled
 * frame as rho[2*v] = Re, rho[2*v + 1] = Im.  md_sq_read waits and returns the number of static samples, s2[nvec],
 * nsamples[nrows] and corr[nrows*nvec] (any pointer may be NULL); md_sq_reset zeroes the accumulators and the counts and
 * keeps the setup and the stored origins.  A slab-decomposition handle, a vector out of range, a slot or row out of
 * range, an empty origin slot and any call before md_sq_setup are refused.                                      */
int md_sq_setup(md_ctx *ctx, const int32_t *n, int nvec, int nslots, int nrows);
int md_sq_sample(md_ctx *ctx, int add_static, const int32_t *slots, const int32_t *rows, int count, int origin_slot);
int md_sq_rho(md_ctx *ctx, double *rho);
int md_sq_read(md_ctx *ctx, int64_t *nstatic, double *s2, int64_t *nsamples, double *corr);
int md_sq_reset(md_ctx *ctx);

/* Pressure tensor and its Green-Kubo correlations, sampled on the device (new relative to the reference, whose users
 * dump frames and recompute every pair force on the host).  One sample evaluates, for the state md_download would return
 * at that moment (unit mass),
 *   K_ab = sum over particles of v_a*v_b                                   (the product rounded, then added)
 *   W_ab = sum over accepted pairs of (f/r)*del_a*del_b,   del = x_j(+periodic translation) - x_i
 * where the accepted pairs are the force kernels': d2 = (del0*del0 + del1*del1) + del2*del2 (no fma) must satisfy
 * d2 <= list_cutoff^2, the potential's own cutoff applies inside the pair evaluation, and f/r is the value the force
 * kernels' generic path uses.  Components, in this order: xx, yy, zz, xy, xz, yz in 3-D (nc = 6); xx, yy, xy in 2-D
 * (nc = 3).  The trace of W_ab is the virial W of md_compute_forces; the pressure tensor is (K_ab + W_ab)/V.
 * Summation: each particle walks its outer neighbour row in row order with t = (f/r)*del_a rounded and
 * W_ab = fma(t, del_b, W_ab) in fp64; then the 64 lanes of a wave (shuffle tree), the 4 waves of a 256-particle block in
 * order, and the blocks in block order (one block, 1024 threads: thread t adds blocks t, t+1024, ..., then the same
 * wave/block tree) -- no floating-point atomics.  Every pair is seen from both ends; the total is multiplied by 0.5
 * (exact).  The tensor therefore depends on the handle's row order: it is reproducible for the same handle history but,
 * unlike the md_dyn_ and md_sq_ samplers' sums, it is not a function of the frame alone (two handles holding the same
 * frame agree to rounding, ~1e-15 of sum |f/r| d2).  Across a periodic face the two ends of a pair see different
 * roundings of the same separation; that residual applies here exactly as it does to the forces.
 *
 * Correlations: md_stress_setup allocates a ring of nlags channel vectors.  Sample number m (0-based since setup or
 * the last reset) forms sig_c = kin_c + vir_c (one rounded add per component) and the channels
 *   3-D: ch0 = sig_xy, ch1 = sig_xz, ch2 = sig_yz, ch3 = (sig_xx - sig_yy)*0.5, ch4 = (sig_yy - sig_zz)*0.5,
 *        ch5 = ((sig_xx + sig_yy) + sig_zz)/3
 *   2-D: ch0 = sig_xy, ch1 = (sig_xx - sig_yy)*0.5, ch2 = (sig_xx + sig_yy)/2
 * stores them in ring[m % nlags], and for k = 0 .. min(m, nlags-1) adds corr[k][ch] += ch(m)*ch(m-k) (the product
 * rounded, then added; no fma; samples in stream order) -- ncorr[k] counts these.  The running sums sum_kin[c] += kin_c,
 * sum_vir[c] += vir_c and nsamples += 1 go with every sample.  The lag unit is the caller's sampling interval.
 *
 * md_stress_setup: 0 <= nlags <= 65536 (0 = tensor and means only); everything zeroed; calling it again starts over.
 * md_stress_sample does not wait and changes nothing the handle computes afterwards: it writes only the sampler's own
 * buffers; if the neighbour list is not valid (first call after md_upload) it builds it exactly as md_compute_forces
 * would, which is the list the next md_run or md_compute_forces would have built itself.  It dispatches on the potential
 * in force at that moment (md_set_potential after the setup is allowed).  md_stress_tensor waits and returns the last
 * sampled frame, kin[nc] and vir[nc].  md_stress_read waits and returns nsamples, sum_kin[nc], sum_vir[nc], ncorr[nlags]
 * and corr[k*nc + ch] (any pointer may be NULL).  md_stress_reset zeroes the sums, corr and the counts and empties the
 * ring; it keeps the setup.  Refused: a slab-decomposition handle, a user potential (MD_POT_CUSTOM), nlags out of range,
 * any call before md_stress_setup, md_stress_tensor before the first sample.                                       */
int md_stress_setup(md_ctx *ctx, int nlags);
int md_stress_sample(md_ctx *ctx);
int md_stress_tensor(md_ctx *ctx, double *kin, double *vir);
int md_stress_read(md_ctx *ctx, int64_t *nsamples, double *sum_kin, double *sum_vir, int64_t *ncorr, double *corr);
int md_stress_reset(md_ctx *ctx);

/* Bond-orientational order, sampled on the device (new relative to the reference, whose users dump frames to learn
 * whether the system crystallised): Steinhardt q_l and its neighbour-averaged (Lechner-Dellago) form for l = 4 or 6 in
 * 3-D, the k-fold psi_k (1 <= k <= 12) in 2-D, and ten Wolde's solid-bond count.  The potential is never evaluated: the
 * sampler serves every potential, MD_POT_CUSTOM included.
 *
 * Neighbours: j is a neighbour of i iff d2 < rn2, with del = x_j(+periodic translation) - x_i as the force kernels form
 * it, d2 = (del0*del0 + del1*del1) + del2*del2 (no fma) and rn2 = r_neigh*r_neigh rounded once on the host;
 * 0 < r_neigh <= list_cutoff (the rows are complete only up to list_cutoff).  n_i = number of neighbours of i.
 *
 * 3-D, u = del/|del|:  Y_lm(u) = sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) P_l^m(cos theta) e^{i m phi}, Condon-Shortley phase,
 * evaluated in fp64 as c_lm D_l^m(u_z) (u_x + i u_y)^m, D_l^m = d^m P_l/dz^m, c_lm = (-1)^m times the square root above.
 * Only m = 0..l is stored (NM = l + 1 complex numbers per particle); Y_{l,-m} = (-1)^m conj(Y_lm).
 *   q_lm(i) = (1/n_i) sum_j Y_lm(u_ij)   (0 if n_i = 0)
 *   q_l(i)  = sqrt(4 pi/(2l+1) (|q_l0|^2 + 2 sum_{m>0} |q_lm|^2))
 *   Q_lm(i) = (q_lm(i) + sum_{j in N(i)} q_lm(j))/(n_i + 1),   qbar_l(i) = the same invariant of Q_lm
 *   s_ij    = Re sum_{m=-l..l} q_lm(i) conj(q_lm(j)) / (|q_l(i)| |q_l(j)|), |.| the 2-norm over all m (0 if either is 0)
 *   c_i     = number of neighbours with s_ij > threshold;  i is solid iff c_i >= min_conn
 * 2-D (NM = 1): psi_k(i) = (1/n_i) sum_j ((del_x + i del_y)/|del|)^k, the invariant is |psi_k(i)|; Q, qbar and s_ij are
 * the same formulas with that single component.
 *
 * The frame vector fr[8]: sum_i q, sum_i q^2, sum_i qbar, sum_i qbar^2, sum_i n_i, sum_i c_i, the number of solid
 * particles, and the global order parameter sqrt(4 pi/(2l+1) sum_m |sum_i n_i q_lm(i) / sum_i n_i|^2)  (2-D:
 * |sum_i n_i psi_k(i) / sum_i n_i|).  Summation: each particle walks its outer neighbour row in row order; then the 64
 * lanes of a wave, the 4 waves of a block in order and the blocks in block order -- no floating-point atomics.  The
 * per-particle sums depend on the handle's row order: reproducible for one handle history, not a function of the frame
 * alone (two handles holding the same frame agree to rounding, ~1e-14).
 *
 * Accumulated on the device since setup or the last reset: sum_fr[8] += fr and nsamples; integer histograms
 * hist_q[nbins], hist_qbar[nbins] over [0, 1], bin = min((int)(value*nbins), nbins-1); hist_nnb[33] and hist_conn[33],
 * counts of n_i and c_i clamped to 32; sample number m < nseries also writes fr into series[m*8 .. m*8+8).
 *
 * md_boo_setup: order = l (4 or 6) in 3-D, k (1..12) in 2-D; 1 <= nbins <= 8192; threshold finite; 0 <= min_conn <= 32;
 * 0 <= nseries <= 2^20; everything zeroed; calling it again starts over.  md_boo_sample does not wait and changes nothing
 * the handle computes afterwards: it writes only the sampler's own buffers; if the neighbour list is not valid (first
 * call after md_upload) it builds it exactly as md_compute_forces would.  md_boo_particles waits and returns the last
 * SAMPLED frame in particle-id order, whatever the handle did since (md_run, list rebuilds, md_upload): nnb[N], q[N],
 * qbar[N], nconn[N] (any may be NULL).  md_boo_qlm waits and returns
 * qlm[(i*NM + m)*2 + {0, 1}] = Re, Im of q_lm(i) of the last frame.  md_boo_read waits and returns nsamples, sum_fr[8],
 * the four histograms and series[nseries*8] (rows past nsamples are zero; any pointer may be NULL).  md_boo_reset zeroes
 * the sums, the histograms, the series and the count; it keeps the setup.  Refused: a slab-decomposition handle,
 * r_neigh > list_cutoff, an argument out of range, any call before md_boo_setup, md_boo_particles or md_boo_qlm before
 * the first sample.                                                                                                  */
int md_boo_setup(md_ctx *ctx, double r_neigh, int order, int nbins, double threshold, int min_conn, int64_t nseries);
int md_boo_sample(md_ctx *ctx);
int md_boo_particles(md_ctx *ctx, int32_t *nnb, double *q, double *qbar, int32_t *nconn);
int md_boo_qlm(md_ctx *ctx, double *qlm);
int md_boo_read(md_ctx *ctx, int64_t *nsamples, double *sum_fr, int64_t *hist_q, int64_t *hist_qbar, int64_t *hist_nnb,
                int64_t *hist_conn, double *series);
int md_boo_reset(md_ctx *ctx);

/* Clusters, sampled on the device (new relative to the reference): the connected components of the bond graph over the
 * member particles -- every particle's cluster, the cluster-size histogram, the largest cluster n_max (with
 * MD_CLUSTER_SOLID ten Wolde, Ruiz-Montero and Frenkel's largest solid cluster).  The potential is never evaluated.
 *
 * Members.  MD_CLUSTER_ALL: every particle.  MD_CLUSTER_SOLID: particle id p is a member iff nconn(p) >= min_conn in the
 * last frame md_boo_sample took; membership is carried by particle id, so what the handle did between the two samples
 * (md_run, list rebuilds) does not matter.  Take both samples at the same step to get ten Wolde's cluster.
 *
 * Bonds.  Members a != b are bonded iff d2 < rb2, with del = x_b(+periodic translation) - x_a as the force kernels form
 * it, d2 = (del0*del0 + del1*del1) + del2*del2 (no fma) and rb2 = r_bond*r_bond rounded once on the host;
 * 0 < r_bond <= list_cutoff (the rows are complete only up to list_cutoff).  A periodic image of a particle is that
 * particle; an image of the particle itself is ignored.  Clusters are the connected components; a cluster that reaches
 * its own periodic image is one cluster (spanning is not detected).
 *
 * Per particle, of the last sampled frame: label[p] = the smallest particle id in p's cluster, size[p] = that cluster's
 * size; a non-member has label -1 and size 0.
 *
 * The frame vector fr[8], all int64: 0 members; 1 clusters; 2 the largest cluster's size; 3 the second-largest's (equal to
 * the largest on a tie, 0 if there is one cluster or none); 4 the sum over members of the degree (directed bonds);
 * 5 sum over clusters of size^2; 6 the label of the largest cluster (the smallest label among ties, -1 if there is no
 * member); 7 clusters of size 1.  Every entry is an integer and a function of the frame alone: the same bits for any
 * handle history, row order or slot order.
 *
 * Accumulated on the device since setup or the last reset: sum_fr[8] += fr (the sum of entry 6 has no meaning) and
 * nsamples; hist_size[max_size+1]: += 1 at index min(size, max_size) for every cluster (entry 0 stays 0, the last entry
 * also holds everything larger); sample number m < nseries also writes fr into series[m*8 .. m*8+8).
 *
 * md_cluster_setup: members = MD_CLUSTER_ALL or MD_CLUSTER_SOLID; 1 <= max_size <= 65536; 0 <= nseries <= 2^20;
 * everything zeroed; calling it again starts over.  md_cluster_sample does not wait and changes nothing the handle
 * computes afterwards: it writes only the sampler's own buffers; if the neighbour list is not valid it builds it exactly
 * as md_boo_sample does.  md_cluster_particles waits and returns the last SAMPLED frame in particle-id order, whatever
 * the handle did since (md_run, list rebuilds, md_upload): label[N], size[N] (either may be NULL).  md_cluster_read waits
 * and returns nsamples, sum_fr[8], hist_size[max_size+1] and series[nseries*8] (rows past nsamples are zero; any pointer
 * may be NULL).  md_cluster_reset zeroes the sums, the histogram, the series and the count; it keeps the setup.
 * Refused: a slab-decomposition handle, r_bond out of range, an unknown `members`, an argument out of range, any call
 * before md_cluster_setup, md_cluster_particles before the first sample; with MD_CLUSTER_SOLID md_cluster_setup before
 * md_boo_setup and md_cluster_sample before the first md_boo_sample.                                                   */
#define MD_CLUSTER_ALL   0
#define MD_CLUSTER_SOLID 1
int md_cluster_setup(md_ctx *ctx, double r_bond, int members, int max_size, int64_t nseries);
int md_cluster_sample(md_ctx *ctx);
int md_cluster_particles(md_ctx *ctx, int32_t *label, int32_t *size);
int md_cluster_read(md_ctx *ctx, int64_t *nsamples, int64_t *sum_fr, int64_t *hist_size, int64_t *series);
int md_cluster_reset(md_ctx *ctx);

/* Cage-relative dynamics and bond breaking, sampled on the device (new relative to the reference): displacements measured
 * relative to the neighbours a particle had at the time origin -- free of the long-wavelength (Mermin-Wagner) drift that
 * makes the plain MSD and F_s of md_dyn_* decay in 2-D although nobody left its cage -- and the bond-breaking
 * correlation C_B(t) of Yamamoto and Onuki.  The potential is never evaluated.
 *
 * Bond criterion.  sigma_ij = (sigma_i + sigma_j) / 2.0.  A radius r is passed iff d2 < (r*s)*(r*s) with s = sigma_ij if
 * `scaled`, else 1.0; d2 = (b0*b0 + b1*b1) + b2*b2 (no fma) of the vector b in question; fp64 throughout.
 *
 * md_cage_origin(slot) stores the current frame (md_dyn_origin's: wrapped x, images, particle-id order) and the
 * neighbour table of the slot: for every particle i, in the order of its neighbour-list row, the entries (j, del_ij) of
 * the row's entries that pass the criterion with r_neigh; del_ij = x_j(+periodic translation) - x_i as the force kernels
 * form it.  A neighbour is a (particle, periodic image) pair: in a small cell j may appear through two images.
 * n_i = min(hits, max_neigh); every hit beyond max_neigh is dropped and counted in `overflow`.  The diameters are the
 * origin's.  The table is keyed by particle id: list rebuilds and md_upload do not touch a stored origin.  If the
 * neighbour list is not valid the call builds it exactly as md_boo_sample does.  It does not wait.
 *
 * md_cage_sample(slots, rows, count) exports the current frame once and, per (slot, row):
 *   Del_i      the displacement since the slot's origin, by md_dyn_sample's formula
 *   m_i        = (sum over i's entries k, in order, of Del_{j_k}) / n_i
 *   Del^CR_i   = Del_i - m_i;  d2 = |Del^CR_i|^2, d4 = d2*d2, s_i(q) = sum over the axes c of cos(q*Del^CR_c)
 *   bond k of i at the sample time: b = del_ij + (Del_j - Del_i) -- exact under any number of boundary crossings; it
 *              survives iff it passes the criterion with r_break, else it is broken
 * A particle with n_i = 0 contributes to nothing.  Added into the row, since setup or the last reset:
 *   sums[row*(2+nq)]   sum d2, sum d4, sum s(q_0..): fp64, reduced over particle ids in md_dyn's fixed tree (no
 *                      floating-point atomics: the same two frames and table give the same bits)
 *   counts[row*3]      particles with n_i > 0, sum n_i, surviving bonds (directed)
 *   hist_broken[row*33] particles with n_i > 0 by their number of broken bonds, 0..32
 *   nsamples[row] += 1
 * The integers are functions of the two frames alone; the fp64 sums depend on the row order the origin was stored with
 * and agree across handles to rounding.  Neither call writes anything of the handle: a run with samples is bit-identical
 * to one without.  md_cage_particles waits and returns, in particle-id order, n_i, d2 of Del^CR_i and the broken count
 * of the last (slot, row) of the last md_cage_sample call (any may be NULL; 0 where n_i = 0).  md_cage_read waits and
 * returns nsamples[nrows], sums, counts, hist_broken and overflow[1] (any may be NULL).  md_cage_reset zeroes the rows; it
 * keeps the setup, the stored origins and -- because it belongs to them -- overflow.
 *
 * md_cage_setup: 1 <= nslots <= 64; nrows >= 1; finite 0 < r_neigh <= r_break; scaled 0 or 1; 1 <= max_neigh <= 32;
 * 0 <= nq <= 16 finite q; allocates the table, nslots*N*max_neigh*(4+8*d) bytes, and zeroes everything; calling it again
 * starts over.  MDHIP_CAGE_ALLOC_LIMIT=bytes in the environment refuses a larger table as a failed allocation is
 * refused.  Refused: a slab-decomposition handle, an argument out of range, a failed table allocation, any call before
 * md_cage_setup, a slot or row out of range, an empty slot, md_cage_particles before the first sample, and
 * md_cage_origin when r_neigh (times the largest diameter if scaled) exceeds list_cutoff: the rows are complete only up
 * to it.                                                                                                              */
int md_cage_setup(md_ctx *ctx, int nslots, int nrows, double r_neigh, double r_break, int scaled, int max_neigh,
                  const double *q, int nq);
int md_cage_origin(md_ctx *ctx, int slot);
int md_cage_sample(md_ctx *ctx, const int32_t *slots, const int32_t *rows, int count);
int md_cage_particles(md_ctx *ctx, int32_t *nnb, double *d2cr, int32_t *broken);
int md_cage_read(md_ctx *ctx, int64_t *nsamples, double *sums, int64_t *counts, int64_t *hist_broken, int64_t *overflow);
int md_cage_reset(md_ctx *ctx);

/* Four-point dynamics, sampled on the device (new relative to the reference): the self overlap Q(t0, t) = sum_i w_i with
 * w_i = 1 iff particle i moved less than `a` between the origin t0 and t0 + t, the moments of Q behind the four-point
 * susceptibility chi4(t) = (<Q^2> - <Q>^2) / N, and the structure factor of the slow particles
 * S4(q, t) = <|W(q)|^2> / N, W(q) = sum_i w_i exp(+i q.x_i(t0)) (Lacevic, Starr, Schroder, Glotzer 2003), on md_sq_setup's
 * wave vectors q_n = 2 pi U^-T n.  The potential is never evaluated.
 *
 * md_chi4_origin(slot) stores md_dyn_origin's frame (wrapped x and int32 images in particle-id order, written by the step
 * loop's own export) and, if nvec > 0, md_sq_sample's f = U^-1 x of that frame, one array per axis: a slot is N*d*20
 * bytes with vectors and N*d*12 without.  It does not wait and writes nothing of the handle.
 *
 * md_chi4_sample(slots, rows, count) exports the current frame once and, per (slot, row) in call order:
 *   Del_i, d2   the displacement since the slot's origin and its square, exactly md_dyn_sample's (no fma)
 *   w_i         = 1 iff d2 < a2, a2 = a*a formed once at setup in fp64; strict: d2 == a2 is not slow
 *   Q           = sum_i w_i, an integer
 *   W[v]        = sum over i with w_i = 1 of (cos 2 pi r, sin 2 pi r), the phase md_sq_sample's evaluated on the ORIGIN
 *                 frame's f: t = (n_0 f_0 + n_1 f_1) + n_2 f_2, r = t - rint(t), the same polynomials; summed in
 *                 md_sq_sample's tree, fixed by N alone (thread: 16 ids in order; shuffle tree; the 4 waves in order; lane l
 *                 of the reducer takes blocks l, l + 64, ... in order), a fast particle contributing nothing (+0.0); no
 *                 floating-point atomics, so the same two frames give the same bits on any handle.
 *                 |W_device - W_true| <= N*(32*kappa*|n|_1 + 128)*2^-53 per component (md_sq_sample's bound and
 *                 derivation), W_true the extended-precision sum over the same slow set from the same fp64 origin frame
 * and adds into the row, since setup or the last reset:
 *   sum_q[row] += Q;  sum_q2[row] += Q*Q;  nsamples[row] += 1        (integers: functions of the two frames alone)
 *   s4[row*nvec + v] = s4[row*nvec + v] + (Re*Re + Im*Im)            (no fma, in call order)
 * Two samples of one call on the same row are both added.  It does not wait and writes nothing of the handle: a run with
 * origins and samples is bit-identical to one without.
 *
 * md_chi4_last waits and returns, of the last (slot, row) of the last md_chi4_sample call, Q, W as w[2v] = Re,
 * w[2v+1] = Im, and slow[N], w_i as one byte per particle id (any may be NULL).  md_chi4_read waits and returns
 * nsamples[nrows], sum_q[nrows], sum_q2[nrows] and s4[nrows*nvec] (any may be NULL).  md_chi4_reset zeroes the rows; it
 * keeps the setup and the stored origins.
 *
 * md_chi4_setup: finite a > 0; 0 <= nvec <= 4096 vectors n[nvec*d] under md_sq_setup's rules (|n_c| <= 32767, n != 0);
 * nvec = 0 samples Q only (no f is stored, no mode kernel runs); 1 <= nslots <= 64; nrows >= 1; allocates the slots and
 * zeroes everything; calling it again starts over.  MDHIP_CHI4_ALLOC_LIMIT=bytes in the environment refuses a larger slot
 * allocation as a failed allocation is refused (the message names the byte count).  Refused: a slab-decomposition handle,
 * an argument out of range, a failed allocation, any call before md_chi4_setup, a slot or row out of range, an empty slot,
 * md_chi4_last before the first sample, and a sample that could let sum_q2 overflow: the library counts the samples of a
 * row and refuses the whole call when (nsamples[row] + 1)*N*N > 2^63 - 1 (read and reset first).                       */
int md_chi4_setup(md_ctx *ctx, double a, const int32_t *n, int nvec, int nslots, int nrows);
int md_chi4_origin(md_ctx *ctx, int slot);
int md_chi4_sample(md_ctx *ctx, const int32_t *slots, const int32_t *rows, int count);
int md_chi4_last(md_ctx *ctx, int64_t *q, double *w, void *slow /* uint8_t[N] */);
int md_chi4_read(md_ctx *ctx, int64_t *nsamples, int64_t *sum_q, int64_t *sum_q2, double *s4);
int md_chi4_reset(md_ctx *ctx);

/* Current correlations and the velocity autocorrelation, sampled on the device (new relative to the reference, whose
 * users dump positions and velocities and redo the sums on the host).  A frame is what md_download returns at that
 * moment: wrapped x and v in particle-id order, written by the same gather into buffers the sampler owns.  On
 * md_sq_setup's integer wave vectors n (the same limits), the particle current is
 *   j_a(n) = sum over particles of v_a exp(+i q_n.x),  a = 0..d-1,
 * with md_sq_sample's phase, operation for operation (f, t = (n_0*f_0 + n_1*f_1) + n_2*f_2, r = t - rint(t), then the
 * same cos 2*pi*r, sin 2*pi*r); the particle adds fma(v_a, cos, Re j_a) and fma(v_a, sin, Im j_a), all in fp64.  The sum
 * over particles is md_sq_sample's tree, fixed by N alone, without floating-point atomics: j is a function of the frame
 * only (the same bits on any handle), and per vector, component a and part
 *   |j_a - j_a,true| <= V_a * (32*kappa*|n|_1 + 128) * 2^-53,   V_a = sum_i |v_i,a|,  kappa as for md_sq_sample.
 * Accumulators, fp64, no fma, added in stream order, with the caller's direction e[v*d + a] per vector (finite, not all
 * zero; the unit vector q_n/|q_n| for the longitudinal / transverse split) and pL = (e_0*j_0 + e_1*j_1) + e_2*j_2 formed
 * for Re and Im separately (2-D: no third term):
 *   static                 s_tot[v]  += sum over a, in order, of (Re_a*Re_a + Im_a*Im_a);  s_long[v] += pL_re^2 + pL_im^2
 *   frame vs slot s, row k c_tot[k][v] += sum over a, in order, of (Re_a*oRe_a + Im_a*oIm_a)
 *                          c_long[k][v] += pL_re*oL_re + pL_im*oL_im   (oL: the same expression of the stored origin j)
 * so C_L = c_long/(ns*N) and C_T = (c_tot - c_long)/((d-1)*ns*N).  An origin is the frame's j, 2*d*nvec doubles.
 *
 * With vacf != 0 an origin also stores the frame's velocities (N*d doubles per slot), and every (slot, row) pair adds
 *   Z = sum over particles of (v_0*o_0 + v_1*o_1) + v_2*o_2     (no fma; 2-D: no third term)
 * to z[row], reduced in a tree fixed by N alone (thread: 4 ids in order; shuffle tree; the 4 waves in order; one reduce
 * block: thread t sums the blocks t, t + 1024, ..., a shuffle tree per wave and one over the 16 waves), no atomics, the
 * totals added in call order; |Z - Z_true| <= A*64*2^-53, A = sum_i sum_a |v_i,a(t)*v_i,a(t0)|.  A static sample adds
 * the same sum of the frame against itself (the equal-time Z) to z[nrows], the row after the lag rows.
 *
 * md_cur_setup: nvec vectors n[nvec*d] and directions e[nvec*d] under md_sq_setup's rules (1 <= nvec <= 16384; nvec = 0
 * is allowed with vacf != 0 and samples Z only), 0 <= nslots <= 64, nrows >= 0, vacf 0 or 1; everything zeroed; calling
 * it again starts over.  MDHIP_CUR_ALLOC_LIMIT=bytes in the environment refuses a larger velocity-slot allocation as a
 * failed allocation is refused.  md_cur_sample exports the frame once, evaluates j once, then, in this order: adds the
 * static sample if add_static != 0, adds the `count` correlations (frame vs slots[i] into rows[i]) in call order, and
 * stores the origin (j and, with vacf, the velocities) in origin_slot unless that is -1 -- a slot may be read and
 * overwritten in one call.  It does not wait and changes nothing the handle computes afterwards.  md_cur_last waits and
 * returns j of the last sampled frame, j[(v*d + a)*2 + {Re, Im}].  md_cur_read waits and returns the number of static
 * samples, s_tot[nvec], s_long[nvec], nsamples[nrows], c_tot[nrows*nvec], c_long[nrows*nvec] and z[nrows + 1] (any may be
 * NULL; z != NULL without vacf is refused); md_cur_reset zeroes the accumulators and the counts and keeps the setup and
 * the stored origins.  Refused: a slab-decomposition handle, a vector, slot or row out of range, an empty origin slot,
 * any call before md_cur_setup, md_cur_last before the first sample.                                              */
int md_cur_setup(md_ctx *ctx, const int32_t *n, const double *e, int nvec, int nslots, int nrows, int vacf);
int md_cur_sample(md_ctx *ctx, int add_static, const int32_t *slots, const int32_t *rows, int count, int origin_slot);
int md_cur_last(md_ctx *ctx, double *j);
int md_cur_read(md_ctx *ctx, int64_t *nstatic, double *s_tot, double *s_long, int64_t *nsamples, double *c_tot,
                double *c_long, double *z);
int md_cur_reset(md_ctx *ctx);

/* Marked pair correlations, sampled on the device: the spatial correlation of a per-particle field -- the orientational
 * correlation g6(r) = <psi6(i) psi6*(j) delta(r - r_ij)> in 2-D, G_l(r) built from q_lm in 3-D, or any field the caller
 * uploads (velocities, displacements, mobility: C_vv(r), the displacement correlations behind chi4).
 *
 * Definition.  Every particle carries NC real marks a_c(i); there are NC weights w_c.  For the unordered pair {i, j}
 * p_c = a_c(i)*a_c(j) (one product: the same whichever particle is visited first) and t_ij is the chain
 * acc = 0; for c = 0..NC-1: acc = fma(w_c, p_c, acc).  The pair's distance, periodic translation and bin are md_rdf's,
 * operation for operation: d2 = (del0*del0 + del1*del1) + del2*del2 with the end of the larger particle id translated,
 * bin k iff e2[k] <= d2 < e2[k+1] on the table e2[k] = (k*delta)^2, delta = r_max / nbins; every face distance must be
 * >= 3*r_max.  The pair contributes the integer I_ij = llrint(t_ij * 2^31 / tmax); tmax is rounded up to a power of two
 * by md_mpc_setup, so the scaling is exact.  Per bin and per sample the device forms cnt[k] (the number of pairs) and
 * sum[k] = sum I_ij, and per sample self = sum_i I_ii.  These are integers: the result does not depend on the order in
 * which the pairs are visited, the launch shape or what the handle did before -- given the frame and the marks it is a
 * function of those alone.  The quantum is tmax * 2^-31; quantisation moves sum/cnt by at most tmax * 2^-32.
 *
 * range_error is sticky until md_mpc_setup or md_mpc_reset: bit 0 (1) -- a term with |t| > tmax*(1 + 2^-10), which
 * contributes 0 to sum and 1 to cnt; bit 1 (2) -- a bin with cnt[k] >= 2^31 in one sample.  Nothing wraps silently: with
 * both absent |sum[k]| < 2^63.
 *
 * Accumulated since setup or reset: acc_cnt[k] (integers), acc_sum[k] and acc_self (doubles: acc = acc + (double)sum,
 * one conversion and one add per sample, in sample order) and nsamples.  The last sample's integers stay readable.
 *
 * Sources.  MD_MPC_BOO: the marks are the stored Re, Im of q_lm, m = 0..l, of the bond-order sampler's last frame (3-D:
 * NC = 2(l+1) = 10 or 14; 2-D: psi_k, NC = 2), the weights 4pi/(2l+1) * {1, 1, 2, 2, ...} (2-D: {1, 1}) and tmax = 1,
 * so t_ij = 4pi/(2l+1) * sum_{m=-l..l} q_lm(i) q_lm*(j) <= q_l(i) q_l(j) <= 1 and sum/cnt * 2^-31 is the conventional
 * G_l(r) = g_l(r) / g(r).  nc, weights and tmax are ignored (pass 0, NULL, 0).  The marks are fetched by particle id, so a
 * list rebuild between md_boo_sample and md_mpc_sample cannot attach them to other particles; that the frame belongs
 * to the same step is the caller's business (as for md_cluster_sample with MD_CLUSTER_SOLID).  MD_MPC_USER: the marks
 * marks[i*NC + c] in particle-id order, NC = 1..3, uploaded by md_mpc_marks (which waits) and kept until replaced; the
 * caller gives weights[NC] and tmax.
 *
 * md_mpc_setup: 1 <= nbins <= 4096; everything zeroed; calling it again starts over (user marks included).
 * md_mpc_sample adds one sample of the current positions on the handle's stream, does not wait and changes nothing the
 * handle computes afterwards.  md_mpc_last waits and returns the last sample's cnt[nbins], sum[nbins] and self (any may
 * be NULL).  md_mpc_read waits and returns nsamples, acc_cnt[nbins], acc_sum[nbins], acc_self, the tmax in use and
 * range_error (any may be NULL).  md_mpc_reset zeroes the accumulators, nsamples, the last sample and range_error and
 * keeps the setup and the user marks.  Refused: a slab-decomposition handle, any call before md_mpc_setup, a face
 * distance < 3*r_max, nbins outside 1..4096, nc outside 1..3 (user source), a weight, mark or r_max that is not finite,
 * tmax not finite or <= 0, MD_MPC_BOO before md_boo_setup (at setup) or before the first md_boo_sample (at sample),
 * MD_MPC_USER sampled before md_mpc_marks, md_mpc_marks on an MD_MPC_BOO setup, md_mpc_last before the first sample. */
#define MD_MPC_BOO  0
#define MD_MPC_USER 1
int md_mpc_setup(md_ctx *ctx, int source, double r_max, int nbins, int nc, const double *weights, double tmax);
int md_mpc_marks(md_ctx *ctx, const double *marks);
int md_mpc_sample(md_ctx *ctx);
int md_mpc_last(md_ctx *ctx, int64_t *cnt, int64_t *sum, int64_t *self);
int md_mpc_read(md_ctx *ctx, int64_t *nsamples, int64_t *acc_cnt, double *acc_sum, double *acc_self, double *tmax,
                int32_t *range_error);
int md_mpc_reset(md_ctx *ctx);

/* compute_kinetic: src/thermostat.jl:50-60 */
int md_kinetic(md_ctx *ctx, double *kinetic);

/* Velocity rescale v *= s (the last loop of bussi!, src/thermostat.jl:43-45), exposed for
 * host-driven thermostats. */
int md_scale_velocities(md_ctx *ctx, double s);

/* Instrumentation (not part of the reference surface). */
typedef struct {
    int64_t steps;          /* steps integrated since create */
    int64_t rebuilds;       /* cell/neighbour-list rebuilds */
    int64_t violations;     /* rebuilds triggered by the displacement check (not scheduled) */
    int64_t n_ghost;        /* periodic ghost copies in the last build */
    int64_t max_neighbors;  /* neighbour-list row capacity */
    double avg_neighbors;   /* mean list length of the last build (candidates/particle) */
    int64_t force_launches; /* ORDINARY force / step kernel launches timed since md_profile(ctx, k) (every k-th one) */
    double force_ms;        /* their summed duration, HIP events on the handle's stream */
    int64_t max_halo;       /* largest per-tile halo (LDS-staged neighbours) of the last build */
    int64_t tiled;          /* 1 if the LDS-tiled force kernel is in use, 0 if the global-gather one */
    int64_t prunes;         /* row prunes (inner-list refreshes) since create */
    int64_t kickdrift_launches; /* kick-drift kernel launches timed since md_profile(ctx,1) */
    double kickdrift_ms;        /* their summed duration */
    int64_t fused;          /* 1: the last md_run used the fused step kernel (one launch per step), 0: the classic
                               kick-drift / force sequence */
    int64_t walked_outer;   /* row entries one launch over the OUTER rows walks (wave-padded, summed over particles) */
    int64_t walked_inner;   /* ... over the current INNER rows (0: none valid): the pair evaluations an ordinary step issues */
    int64_t prune_launches_timed; /* PRUNE-step launches timed since md_profile(ctx, k): every one, whatever the stride;
                                     not counted in force_launches */
    double prune_ms;        /* their summed duration */
    int64_t rebuilds_timed; /* list builds timed since md_profile(ctx, k): every one, whatever the stride */
    double rebuild_ms;      /* their summed duration, from the end of the last step before the build to the point where
                               the next step can start (state conversion, sort, gather, rows, host waits included) */
    int64_t fused_build;    /* 1: the rows of the last build came from the fused per-tile kernel (k_build_tile), 0: from the
                               two-kernel fallback (a tile or a cell did not fit it) */
    int64_t own_first;      /* 1: the last step launch took the tile's own records from registers (own-first halo list of
                               k_build_tile), 0: it gathered every record through the halo list */
} md_stats;
/* enable = 0: off; 1: HIP events around every force and kick-drift launch; k > 1: around every k-th launch of each
 * (an event record costs a few microseconds of device time: sampling keeps a timed run honest) */
int md_profile(md_ctx *ctx, int enable);
int md_get_stats(md_ctx *ctx, md_stats *out);

/* The Verlet rows as they are, for audits (tests/row_audit.py): never builds, prunes or changes anything.  Two calls like
 * md_neighbor_pairs: entries = NULL, cap = 0 for *count, then again with room for it.
 *   which    0: the outer rows (cutoff + skin, built at x0); 1: the inner rows (cutoff + inner skin, pruned at x1) -- an
 *            error unless info[6] (inner_valid) is set
 *   info     NULL or MD_LIST_ROWS_INFO doubles:
 *            [0] list cutoff  [1] effective skin (after the box clip)  [2] list radius rl = cutoff + skin
 *            [3] inner skin (0 without valid inner rows)  [4] d1 = max |x1 - x0| as the prune step measured it (Euclidean)
 *            [5] list_valid  [6] inner_valid  [7] tiled (16-bit rows into per-tile halo lists)  [8] fused build
 *            (k_build_tile; 0 with [7] set: the two-kernel fallback)  [9] own-first halo numbering  [10] the inner rows
 *            index the inner halo image  [11] n  [12] rows are 32-bit global slots (no tiles)  [13] real ghost slots
 *            [14] halo words carry owner | shift code (virtual ghosts)  [15] this build supports inner rows
 *   entries  cap x 5 int32, one (id_i, id_j, n_0, n_1, n_2) per row entry, rows in slot order, every row in row order,
 *            both directions of a pair (j in the row of i, and i in the row of j).  n in {-1, 0, 1}^d is the periodic image
 *            the entry stands for: the record the pair loop reads is x_j + n . A (A: columns = lattice vectors).
 *            Sentinel / padding entries are left out.  An entry that cannot be decoded has id_j = -1 or an image
 *            component of 2.
 *   x0, x1, pos   all NULL, or n x d each by particle id (the layout of md_download), in the handle's own unwrapped frame:
 *            positions at the last list build, at the last prune (== x0 without valid inner rows), and now.
 * A handle whose rows are not valid (after md_upload, md_run_brownian, md_fire_minimize, ...) reports info with
 * list_valid = 0 and *count = 0.  Slab-decomposition handles are refused. */
#define MD_LIST_ROWS_INFO 16
int md_list_rows(md_ctx *ctx, int which, double *info, int32_t *entries, int64_t cap, int64_t *count, double *x0,
                 double *x1, double *pos);

/* ---------------------------------------------------------------------------------------------
 * Slab decomposition: one handle per GPU, each owning the particles of one slab of the x axis
 * (new relative to the reference, which is single-process).  y and z
 * stay periodic inside the handle; x-direction ghosts are copies of the neighbour slabs'
 * particles.  Two ways to move the data between the ranks:
 *   * the library does it itself on its own RCCL communicator (md_dom_comm_init, then md_dom_rebuild for a whole
 *     list build and md_dom_run_window for a window of steps: no host code between the phases) -- the default of
 *     moleculardynamics/jl_amd/domain.py and bench.py with one GPU per rank;
 *   * the library only packs and unpacks and the CALLER moves the buffers (any transport: the phase-by-phase entry
 *     points below; domain.py drives them through torch.distributed when the native transport is not available).
 *
 * Phase by phase, a list build is the sequence  migrate_pack -> [exchange] -> migrate_unpack -> halo_pack ->
 * [exchange] -> halo_unpack -> build ; a step is  step_begin -> [exchange] -> step_end .
 * side 0 = the left neighbour (rank-1 mod P), side 1 = the right neighbour.  A message sent
 * to side s arrives in the neighbour's receive buffer 1-s.  Record sizes in doubles:
 * migrants 14, halo records 5, per-step halo coordinates 3.
 * ------------------------------------------------------------------------------------------- */
int md_create_domain(int dim, int64_t n_global, int64_t n_cap, const double *box, double list_cutoff,
                     int device_id, int rank, int nranks, md_ctx **out);
int md_dom_set_uniform(md_ctx *ctx, int uniform, double sigma);
/* per-rank state in local order: row k of x/v/f/images belongs to particle ids[k] */
int md_dom_upload(md_ctx *ctx, int64_t n_own, const int32_t *ids, const double *x, const double *v, const double *f,
                  const int32_t *images, const double *diameters);
int md_dom_download(md_ctx *ctx, int64_t cap, int64_t *n_own, int32_t *ids, double *x, double *v, double *f,
                    int32_t *images);
int md_dom_migrate_pack(md_ctx *ctx, int64_t *nsend /* [2] */);
int md_dom_migrate_unpack(md_ctx *ctx, const int64_t *nrecv /* [2] */);
int md_dom_halo_pack(md_ctx *ctx, int64_t *nsend /* [2] */);
int md_dom_halo_unpack(md_ctx *ctx, const int64_t *nrecv /* [2] */);
int md_dom_build(md_ctx *ctx);
/* Optional zero-copy exchange: device buffers owned by the caller (e.g. torch tensors) that the
 * per-step halo coordinates are packed into / read from directly, instead of the library's own
 * buffers + md_dom_get_sendbuf / md_dom_put_recvbuf.  Each must hold capacity_doubles doubles. */
int md_dom_set_step_buffers(md_ctx *ctx, void *send_left, void *send_right, void *recv_left, void *recv_right,
                            int64_t capacity_doubles);
int md_dom_get_sendbuf(md_ctx *ctx, int side, int64_t ndoubles, void *dst, int dst_is_device);
int md_dom_put_recvbuf(md_ctx *ctx, int side, int64_t ndoubles, const void *src, int src_is_device);
/* first half of a step (pending Bussi rescale, half-kick, drift; src/integrate.jl:8-21); *violated = 1 if
 * some particle of this rank moved skin/2 since the build: every rank must then rebuild before forces */
int md_dom_step_begin(md_ctx *ctx, double dt, int *violated);
/* second half (ghost refresh, forces, second half-kick; src/integrate.jl:28-38); uwk = this rank's {U, W, K} */
int md_dom_step_end(md_ctx *ctx, double dt, int want_uw, double *uwk);
int md_dom_forces(md_ctx *ctx, double dt, int kick, int want_uw, double *uwk);
/* velocity scale to apply in front of the next half-kick (bussi!'s rescale, src/thermostat.jl:43-45) */
int md_dom_set_scale(md_ctx *ctx, double scale);
int md_dom_counts(md_ctx *ctx, int64_t *out /* [8]: n_own, nsend_halo L,R, nrecv_halo L,R, n_ghost, 1 if the tiled
                                                  force kernel is in use, 1 if inner rows are active */);

/* Asynchronous slab stepping -- none of these waits for the device.  The caller enqueues on ONE stream, per
 * step,   md_dom_step_a -> all-reduce(MIN) of *flag_dev + neighbour exchange of the step buffers ->
 *         md_dom_step_b -> all-reduce(SUM) of kuw_dev[3] -> md_dom_step_c
 * (the all-reduce only for MD_NVT or on a step that reports U/W/K; md_dom_step_c only on such a reporting step
 * and on the LAST step of a window -- when it is skipped, the next md_dom_step_a forms the Bussi scale from the
 * reduced sums itself), a whole window of steps at a time, with
 * 0-based step numbers inside the window; ktemp/r1/r2 are indexed by them (same meaning as md_run's).  A
 * displacement violation on any rank at step m reaches every rank through the reduced flag before step m's
 * force evaluation: all later kernels of the window skip themselves on every rank (the single-GPU scheme of
 * md_run, made global).  md_dom_async_end waits, reports m (0x7fffffff = none) and the global {U, W, K};
 * after a violation the caller rebuilds (migrate/halo/build) and calls md_dom_forces for step m.
 * md_set_stream makes the handle launch on the caller's hipStream_t (NULL = its own again), so that
 * stream-ordered RCCL calls interleave with the kernels without host synchronisation.                    */
int md_set_stream(md_ctx *ctx, void *hip_stream);
int md_dom_async_begin(md_ctx *ctx, int64_t nsteps, double dt, int ensemble, double tau, double nf, const double *ktemp,
                       const double *r1, const double *r2, int64_t prune_interval, void *flag_dev /* int32[1] */,
                       void *kuw_dev /* double[3] */);
int md_dom_step_a(md_ctx *ctx, double dt, int step);
int md_dom_step_b(md_ctx *ctx, double dt, int step, int want_uw);
int md_dom_step_c(md_ctx *ctx, int step, int want_uw);
int md_dom_async_end(md_ctx *ctx, int apply_pending_scale, int32_t *first_viol, double *uwk, double *info /* [6] or NULL */);

/* Native transport: the same window of steps run entirely inside the library, which issues the three small
 * collectives of a step itself -- RCCL (over xGMI) on the handle's stream.  RCCL is bound at run time from
 * rccl_path (NULL = "librccl.so"; a PyTorch host passes the copy torch has loaded so that one RCCL lives in
 * the process).  Rank 0 obtains the 128-byte unique id and distributes it by any means; every rank then calls
 * md_dom_comm_init (collective; it ends with an all-reduce self-test).  md_dom_run_window = md_dom_async_begin
 * + nsteps x (step_a, all-reduce MIN, neighbour send/recv, step_b, all-reduce SUM, step_c) + md_dom_async_end;
 * report_last asks for the global U, W of the window's last step.  List builds: md_dom_rebuild (below), or the
 * phase-by-phase sequence with the caller's own transport.                                                       */
int md_dom_comm_unique_id(const char *rccl_path, void *id128);
int md_dom_comm_init(md_ctx *ctx, const char *rccl_path, const void *id128);
/* The whole list-build sequence above (md_dom_migrate_pack ... md_dom_build) in ONE call, the neighbour exchanges (counts,
 * migrants, halo records) on the handle's own communicator: no host code between the phases.  Collective; needs
 * md_dom_comm_init.  With inner rows requested, a rank whose build fell back to the generic rows switches them off on every
 * rank and the build is repeated (md_dom_counts()[7] tells). */
int md_dom_rebuild(md_ctx *ctx);
int md_dom_run_window(md_ctx *ctx, int64_t nsteps, double dt, int ensemble, double tau, double nf, const double *ktemp,
                      const double *r1, const double *r2, int report_last, int apply_pending_scale,
                      int64_t prune_interval, int32_t *first_viol, double *uwk, double *info /* [7] or NULL */);
/* On tiled handles md_dom_run_window runs the FUSED step (csrc/md_domain.hpp: one step kernel + two small launches and two
 * collectives per step; what travels is the boundary particles' state records).
 * DIRECT PEER EXCHANGE: md_dom_comm_init also gives every rank a mailbox in fine-grained device memory, shares it with
 * the other ranks (hipIpc handles, carried by the communicator) and rehearses one exchange; if every rank succeeds,
 * a fused window moves its sums and records as ONE-SIDED STORES into the peers' mailboxes (over xGMI between GPUs) and
 * waits on flags in its own -- no collective call per step, one small launch (k_dom_exchange) instead of two launches
 * and two collectives; info[6] = 2.  Anything that prevents it on any rank (no peer access, MDHIP_DOM_P2P=0, more
 * than 16 ranks, a face with more records than a mailbox plane) leaves all ranks on the collectives.  Waits are bounded
 * (MDHIP_P2P_TIMEOUT_S, default 60 s): a peer that never delivers is an error, not a hang.
 * With the fused step info[6] >= 1 and, after a violation,
 * the state returned is that of the last complete step first_viol - 1: the caller refreshes the rows and resumes AT step
 * first_viol (no md_dom_forces call).  info[6] = 0: the classic sequence ran -- the violating step's drift is applied and
 * md_dom_forces completes it.
 * A fused window refreshes the x-halo particles' state RECORDS, not their coordinates: until the next list build (or a
 * classic step's exchange) md_dom_forces refuses to run -- it would read neighbour coordinates as of the last build.
 * A failure of one rank inside a window aborts the communicator (its peers' collectives return an error instead of
 * waiting) and poisons the flags that rank owns in its peers' mailboxes (their waits end at once with an error); the
 * handle needs md_dom_comm_init again.  Any call that fails inside a fused step loop (md_run,
 * md_dom_run_window) leaves the handle's particle state incomplete: later calls that read it fail until md_upload /
 * md_dom_upload provides x, v and f again.                                                                        */
/* Inner rows (see md_set_inner_skin) on a slab handle.  Every rank must prune at the same steps, so the caller
 * plans the schedule from all-reduced quantities: prune_interval (md_dom_async_begin / md_dom_run_window) = steps
 * between prune steps inside a window (0 = none scheduled); info (md_dom_async_end / md_dom_run_window) returns {1 if the violating step was a prune step, this rank's d1 = max|x - x0| at
 * the last executed prune step, steps since the build at that prune step or -1, 1 if pruning is active,
 * effective skin, effective inner skin}.
 * After a violation: all-reduce(MAX) md_dom_max_disp0; if the outer rows still hold (d0 + inner_skin/2 <=
 * skin/2 and the violating step was not a prune step) call md_dom_invalidate_inner, else rebuild; then
 * md_dom_forces for the violating step.                                                                  */
int md_dom_enable_pruning(md_ctx *ctx, int on);
int md_dom_max_disp0(md_ctx *ctx, double *d0);
int md_dom_invalidate_inner(md_ctx *ctx);

/* Swap Monte Carlo: rounds of diameter exchanges at fixed positions, to be interleaved with blocks
 * of md_run (Berthier, Flenner, Fullerton, Scalliet, Singh, J. Stat. Mech. 2019).  The diameter is pos[].w; the rows do not
 * depend on it (list_cutoff is the caller's number), so no round ever invalidates the list.
 * One ROUND, a function of (positions, diameters, seed, round index) alone:  Philox4x32-10, key = seed, counter =
 * (0-based particle index i, round lo, round hi, 1) gives w0..w3.  i proposes iff w0 < min(2^32 - 1, floor(fraction 2^32));
 * its partner is j = (w1 * N) >> 32 (anywhere in the box; j == i: the proposal is void); the swap's key is (w2 << 32) | i.
 * Both members take the minimum key offered to them; a swap that holds it at both members is live, the others have lost
 * the claim.  A live swap that finds, within list_cutoff of either member, a member of a live swap with a smaller key is
 * blocked (one pass, conservative: it yields even when that swap is blocked itself).  Otherwise: filtered when
 * |sigma_i - sigma_j| > max_diameter_difference (<= 0: no filter), else accepted iff (w3 + 0.5) / 2^32 < exp(-dU / ktemp),
 * dU = sum over the neighbours k != partner of u(r, sigma_partner, sigma_k) - u(r, sigma_self, sigma_k) for both members,
 * pairs and pair energies as md_compute_forces takes them.  An accepted swap exchanges the two diameters.
 * md_swap_setup: fraction in (0, 1].  Single-GPU handles only.
 * md_swap_rounds: rebuilds the list first when it is not valid (as md_compute_forces does), enqueues rounds first_round ..
 * first_round + nrounds - 1 without a host wait in between, then makes every copy of a diameter the handle holds
 * consistent and finishes with one force evaluation, as md_compute_forces: the handle's forces belong to the new diameters
 * and *energy, *virial are their U and W.  counts = {proposed, void, lost the claim, blocked, filtered, accepted} over the
 * call's rounds; *decided = accepted + rejected; *du_accepted = sum of dU over the accepted swaps.  Any output may be NULL.
 * Refused: before md_swap_setup; ktemp <= 0; all diameters equal; MD_POT_CUSTOM -- the pair energy of a run-time compiled
 * potential is not reachable from the swap kernel.
 * md_swap_last: the last round by particle index: partner (-1: i did not propose), status (0 none, 1 void, 2 lost the
 * claim, 3 blocked, 4 filtered, 5 rejected, 6 accepted; at the proposer) and dU (decided swaps, else 0).
 * md_diameters: the current diameters by particle index.                                                              */
int md_swap_setup(md_ctx *ctx, double fraction, double max_diameter_difference /* <= 0: none */, uint64_t seed);
int md_swap_rounds(md_ctx *ctx, int64_t nrounds, double ktemp, int64_t first_round,
                   int64_t *counts /* [6]: proposed, void, lost the claim, blocked, filtered, accepted */,
                   int64_t *decided, double *du_accepted, double *energy, double *virial);
int md_swap_last(md_ctx *ctx, int32_t *partner, int32_t *status, double *du);
int md_diameters(md_ctx *ctx, double *diameters);

/* Hessian of the pair energy on the device (new relative to the reference): the operator H X, its
 * diagonal blocks, and the lowest modes by Lanczos with the basis resident on the device.
 *
 * With U(r) the pair energy, t = U'(r)/r, k = U''(r), n = (x_i - x_j)/r, over the pairs md_compute_forces takes
 * (d2 < the accepted threshold in the reference's form, each potential's own cutoff branch inside):
 *   (H X)_i = sum_j [ (k - t) n (n . (X_i - X_j)) + t (X_i - X_j) ],      H_ii = sum_j [ (k - t) n n^T + t I ].
 * H is the Hessian of the smooth part: the jump of U or U' at a sharp cutoff (plain LJ) contributes nothing.  t and k are
 * analytic for MD_POT_LJ, MD_POT_PSEUDOHS, MD_POT_LJ_MODIFIED (all three modes) and MD_POT_POLYDISPERSE; they belong to the
 * FORCE the library evaluates (t = -f/r, k = -df/dr).
 * Arithmetic: one lane per particle walks its outer neighbour row in row order; per row entry the D x D block
 * h_ab = fma((k - t)/d2, del_a del_b, t delta_ab) is formed once (del_a del_b rounded first, so h is symmetric bit for bit)
 * and applied to X_i - X_j of every vector of the block with fma in component order.  Every pair is evaluated from both
 * members; no atomics.  Both members of a pair use one rounding of the separation (across a periodic face: the lower
 * slot's), so the dense matrix equals its transpose bit for bit, a uniform translation gives exactly 0.0, two calls on one
 * handle are bit-identical, and a column does not depend on the other vectors of its block.
 *
 * md_hess_setup: needs a built-in potential and a single-GPU handle; builds the list if it is not valid (as
 * md_compute_forces would) and freezes the operator on the frame the handle holds.  md_upload, md_run, md_run_brownian,
 * md_fire_minimize, md_swap_rounds, md_set_potential*, md_set_skin / md_set_inner_skin and every list rebuild invalidate
 * it: the other md_hess_ calls then fail until md_hess_setup is called again.  md_compute_forces on a valid list does not.
 * md_hess_apply: X, Y are [m][N][D] by particle index (vector-major; each vector is the D x N column-major matrix the
 * rest of this ABI uses), 1 <= m <= 8; waits.
 * md_hess_blocks: diag[N][D][D] by particle index; waits.
 * md_hess_lanczos: ksteps steps of Lanczos with full reorthogonalisation (classical Gram-Schmidt, two passes, against the
 * D uniform translations and all earlier basis vectors; the dot products of a pass in one kernel, block partials then a
 * fixed-order finish, no floating-point atomics), start vector = Philox4x32-10 words keyed by (seed, particle index)
 * projected against the translations.  The basis (ksteps vectors of N D doubles) stays on the device; when it cannot be
 * allocated the error names the size.  No host wait inside the loop.  Returns alpha[ksteps] (diagonal) and beta[ksteps]
 * (beta[j] couples steps j and j + 1; the last is the residual norm).  1 <= ksteps <= N D - D.
 * md_hess_ritz: Y = V S on the device for S[ksteps][nvec] (row-major; ksteps as in the last md_hess_lanczos), one apply
 * per block of 8; returns modes[nvec][N][D] by particle index and resid[c] = |H y_c - theta[c] y_c|_2.                */
int md_hess_setup(md_ctx *ctx);
int md_hess_apply(md_ctx *ctx, int m, const double *X, double *Y);
int md_hess_blocks(md_ctx *ctx, double *diag);
int md_hess_lanczos(md_ctx *ctx, int ksteps, uint64_t seed, double *alpha, double *beta);
int md_hess_ritz(md_ctx *ctx, int ksteps, int nvec, const double *S, const double *theta, double *modes, double *resid);

/* Elastic moduli of the frame md_hess_setup froze -- meant for a minimum (md_fire_minimize) -- on the device (new relative
 * to the reference): the Born term, the affine force field, and the non-affine term by conjugate
 * gradients around the operator of md_hess_apply.
 *
 * Definitions.  del = x_j(+translation) - x_i, r = |del|, t = U'/r, k = U'', c = (k - t)/r^2, over the pairs of md_hess_*;
 * V = |det(cell)|.  Strain is the Green-Lagrange tensor eta: r'^2 = r^2 + 2 del^T eta del.  eta_ab and eta_ba are ONE
 * tensor component; no engineering factor 2 and no Voigt factor appears anywhere.
 *   stress     sigma_ab  = (1/V) sum_pairs t del_a del_b            (= -W_ab / V of md_stress_*; tension is positive)
 *   Born       CB_abcd   = (1/V) sum_pairs c del_a del_b del_c del_d   (totally symmetric)
 *   affine     Xi_{i,c;ab} = d2U / dx_ic d eta_ab = sum_j [ -c del_a del_b del_c - t (delta_ac del_b + delta_bc del_a) ]
 *   non-affine u_ab = -H^+ Xi_ab  on the space orthogonal to the uniform translations;   N_st = (1/V) Xi_s . u_t
 *   moduli     C = CB + N = (1/V) d2 U_min / d eta d eta along the relaxed path (the caller adds; see vibrations.py)
 * Like H these belong to the smooth part of the energy: a jump of U or U' at a sharp cutoff contributes nothing.
 * Components, everywhere: 3-D xx, yy, zz, xy, xz, yz (nc = 6); 2-D xx, yy, xy (nc = 3) -- md_stress_tensor's order.
 * Arrays [nc][nc] are row-major tensor components C_{(ab)(cd)}.
 *
 * md_elas_affine: one lane per particle walks its outer row in row order and adds, per accepted pair, its Xi term and its
 * half of the stress and Born sums (fma, fp64, no atomics); both members of a pair use the same separation bits (md_hess_*),
 * so their Xi terms are exact negatives.  The sums: lanes by block_sum, blocks in block order, times 0.5 (exact) and 1/V
 * once; born[s][t] is filled from the one sum of its sorted index set, so born equals its transpose bit for bit.  Like the
 * stress tensor the sums depend on the row order: bit-reproducible on one handle, equal to rounding across handles; Xi of a
 * particle is a function of the frame and of its row order.  stress[nc], born[nc][nc]; xi is [nc][N][D] by particle index
 * or NULL.  Waits.
 * md_elas_solve: needs md_elas_affine of the SAME md_hess_setup.  Column-wise conjugate gradients for the nc right-hand
 * sides at once, all vectors resident: per iteration one block apply of H, p . H p and r . r by chunk partials and a
 * fixed-order finish that forms alpha_c and beta_c on the device, x += alpha p and r -= alpha H p in one kernel, p = r +
 * beta p in one; no floating-point atomics; the host polls the device-side status once per 32 iterations.  A column is
 * frozen once |r_c| <= tol |Xi_c| (its iteration count is kept) or once p . H p <= 0 (MD_ELAS_INDEFINITE).  The right-hand
 * side and the solution are projected once each against the uniform translation of the particles that have a bond; a
 * particle without one (a zero row of H, zero Xi) gets exactly 0.0.  Returns per column iters[nc], resid[nc] = the TRUE
 * |H u_c + Xi_c|_2 from one more apply, xi_norm[nc] = |Xi_c|_2 (projected); *status = MD_ELAS_CONVERGED (every column met
 * tol) | MD_ELAS_MAX_ITER (some column still iterating after max_iter) | MD_ELAS_INDEFINITE; nonaffine[nc][nc] = N_st, not
 * symmetrised (N - N^T measures the solve's error); u is [nc][N][D] by particle index or NULL.  tol > 0, max_iter >= 1.
 * A saddle or non-convergence is reported in *status, not as an error.  Waits.
 * Both need a frozen operator, a built-in potential and a single-GPU handle, and fail like md_hess_apply otherwise:
 * whatever invalidates the operator invalidates both until md_hess_setup is called again.                              */
#define MD_ELAS_CONVERGED 1
#define MD_ELAS_MAX_ITER 2
#define MD_ELAS_INDEFINITE 4
int md_elas_affine(md_ctx *ctx, double *stress, double *born, double *xi);
int md_elas_solve(md_ctx *ctx, double tol, int64_t max_iter, int64_t *iters, double *resid, double *xi_norm, int *status,
                  double *nonaffine, double *u);

/* Change the unit cell of a live handle and carry the particles along (new relative to the reference, which fixes the cell
 * at initialisation).  box is d x d column-major, columns = lattice vectors, validated and inverted
 * exactly as md_create does; a diagonal matrix takes the orthorhombic fast paths again, anything else is a general cell.
 *
 * MD_CELL_AFFINE: fractional coordinates are kept.  One pass over the state records: frac = U_old^-1 x (invL * x per
 * component, or row times vector left to right, every operation rounded, no fma: the wrap's arithmetic), n = floor(frac),
 * img += n, x = U_new (frac - n) in the new cell's form of that product -- wrap_to_box (src/boundary.jl:7-17) with the old
 * inverse and the new matrix.  frac + img is kept exactly.  Velocities are left as they are; FORCES ARE LEFT STALE (those of
 * the old cell) until the next evaluation (md_compute_forces, md_run, md_fire_minimize, ...).
 * MD_CELL_LATTICE: the new cell must generate the same lattice.  M = U_old^-1 U_new must be integer to 1e-9 per entry
 * (entries up to 2^10), |det M| = 1, and U_old M must give back U_new to 8 ulp of the largest term of each entry's sum.
 * Cartesian positions do not move but for the wrap into the new cell (as md_download wraps: only a coordinate outside
 * [0, 1) moves); img' = M^-1 img in integer arithmetic, plus the wrap's shift.  x + U img is kept to rounding.  A mark of
 * md_nonaffine_mark is carried into the new basis by the same integer matrix.  Refused when an image count (of the state or
 * of the mark) would leave int32: one pass that writes nothing decides that before the pass that writes.
 *
 * Refused, through md_last_error and with the handle's cell and state exactly as before: a singular or non-finite matrix;
 * a face distance below 3 * list_cutoff (what the linked-cell build needs) or below 3 * r_max of md_rdf_ / md_mpc_; a slab
 * handle; a handle whose state a failed step loop left incomplete; a frame in flight (md_snapshot_begin without its _end);
 * a handle with md_dyn_, md_sq_, md_cur_, md_chi4_ or md_cage_ set up (they store time origins, or wave vectors
 * commensurate with the cell the setup saw; the message names the sampler).
 * On acceptance the cell grid is derived again, the ghost capacity and the row capacity follow the new grid and density
 * as in md_create / md_set_skin (buffers only grow), the neighbour lists are invalid (the next evaluation rebuilds), the
 * rebuild schedule measures its displacement rate again, the grids of md_rdf_ / md_mpc_ are derived again, and the frozen
 * operator of md_hess_ / md_elas_ is dropped.  md_rdf_, md_stress_, md_boo_, md_cluster_, md_mpc_ keep working: they
 * read one frame at a time (their running sums then mix cells -- the caller's business).  Waits.
 * A handle on which md_set_cell is never called behaves exactly as before.                                              */
#define MD_CELL_AFFINE 0
#define MD_CELL_LATTICE 1
int md_set_cell(md_ctx *ctx, const double *box, int mode);

/* Displacement since a mark with the affine part taken out (same section).
 * md_nonaffine_mark stores, by particle index, the fractional coordinate U^-1 x (a double) and the image count (an int32)
 * of every particle, separately, so that the image difference is exact.  Allocates N * D * 12 bytes on the first call.
 * md_nonaffine: u_i = U_now ((frac_i - frac0_i) + (img_i - img0_i)).  An affine cell change keeps fractional coordinates,
 * so u is exactly the non-affine part of the displacement since the mark; a lattice change transforms the mark and leaves
 * u unchanged to rounding.  sums[8] = sum u_x, sum u_y, sum u_z (0 in an unused dimension), sum |u|^2, sum |u|^4,
 * max |u|^2, the index of the particle attaining it (the lowest on a tie; as a double), N.  Block partials in a fixed order
 * and a small second pass (one block per sum); the maximum through an integer atomic on the double's bits; no
 * floating-point atomics.  u is [N][D] by particle index or NULL (N * D * 8 bytes more on the first call with u).  Waits.
 * md_nonaffine without a mark, or after md_upload of positions (the mark would describe another frame), is an error.
 * Single-GPU handles only.                                                                                             */
int md_nonaffine_mark(md_ctx *ctx);
int md_nonaffine(md_ctx *ctx, double *sums, double *u);

/* Scale the whole frame of a live handle isotropically and KEEP the Verlet rows (new relative to the reference, which has no
 * barostat).  About the origin of the handle's own unwrapped frame: every entry of the cell matrix is
 * multiplied by mu (one rounding each; the result is validated and inverted exactly as in md_create / md_set_cell), and one
 * pass over the state records does x <- mu x (the diameter untouched), v <- vscale v, one product per component, no fma --
 * numpy's mu * x reproduces both bit for bit.  Image counts, ids and forces are untouched (FORCES ARE THOSE OF THE OLD CELL
 * until the next evaluation, as with md_set_cell); nothing is wrapped, so frac + img is kept up to the rounding of the
 * products and a mark of md_nonaffine_mark stays valid.  The result differs from md_set_cell(mu U, MD_CELL_AFFINE) by
 * rounding only (that one wraps, and goes through fractional coordinates).
 * The rows: the same pass scales the reference positions of the outer rows (x0, list build) and of the inner rows (x1,
 * last prune).  Rows built at radius rl are the rows of radius mu rl in the scaled frame, so they stay, and the step loop
 * gets the skins they still leave beyond the cutoff, which does not scale: with m0 (m1) the product of the factors since the
 * build (the last prune), skin_eff = m0 (cutoff + skin) - cutoff, inner_eff = m1 (cutoff + inner skin) - cutoff, and the
 * displacement d1 between the two reference frames times mu, rounded up.  md_list_rows reports these.  *rows_kept = 1 when
 * the outer rows stayed; 0 when the list was retired and the next evaluation builds in the new cell with the full skin:
 * skin_eff below two thirds of the configured skin, some particle further than skin_eff / 2 from its scaled x0 (measured in the
 * same pass), no valid list, or a handle whose rows are not the tiled two-level kind (user potential, skin 0, rows that do
 * not fit LDS).  The inner rows alone are dropped (the next step prunes) when inner_eff falls below two thirds of the inner skin or a
 * particle is beyond min(inner_eff / 2, skin_eff / 2 - d1) of its scaled x1.  The cell grid of the list, and the buffer
 * capacities that follow it, are derived again at the next build, not here; the grids of md_rdf_ / md_mpc_ are derived
 * again here; the frozen operator of md_hess_ / md_elas_ is dropped; md_stress_, md_boo_, md_cluster_ read the records of
 * the moment.  rows_kept may be NULL.  Waits.
 * Refused, with the handle exactly as before: mu or vscale not finite, mu <= 0; a slab handle; a handle whose state a
 * failed step loop left incomplete; a frame in flight; a new face distance below 3 * list_cutoff, or below 3 * r_max of
 * md_rdf_ / md_mpc_; a handle with md_dyn_, md_sq_, md_cur_, md_chi4_ or md_cage_ set up (the message names the sampler).
 * A handle on which md_scale_cell is never called behaves exactly as before.                                             */
int md_scale_cell(md_ctx *ctx, double mu, double vscale, int *rows_kept);

/* Map the whole frame of a live handle by a deformation gradient F and KEEP the Verlet rows (new relative to the reference,
 * which fixes its cell at initialisation, src/initialization.jl:7-18).  F and G are D x D, row-major;
 * G may be NULL.  About the origin of the handle's own unwrapped frame: the cell becomes F U (row times column, left to
 * right, every product and sum rounded; validated and inverted as in md_create / md_set_cell), and one pass over the state
 * records does x <- F x (the diameter untouched) and, with G, v <- G v: row times vector, left to right, every product and
 * sum rounded, no fma -- the arithmetic of md_set_cell's general branch, which numpy reproduces bit for bit.  G = F^-1 makes
 * the stored velocities peculiar ones (SLLOD).  Image counts, ids and forces are untouched (FORCES ARE THOSE OF THE OLD CELL
 * until the next evaluation); nothing is wrapped, so frac + img is kept up to rounding and a mark of md_nonaffine_mark stays
 * valid.  The result differs from md_set_cell(F U, MD_CELL_AFFINE) by rounding only.
 * The rows: the same pass maps x0 (list build) and, while the inner rows are valid, x1 (last prune).  With M0 (M1) the product
 * of the F's since the build (the last prune), s0 <= sigma_min(M0), s1 <= sigma_min(M1) and S >= sigma_max(F) -- exact
 * singular values from the symmetric eigenproblem of M^T M, widened by a relative 2^-40 in the safe direction --
 *     skin_eff = s0 (cutoff + skin) - cutoff,  inner_eff = s1 (cutoff + inner skin) - cutoff,  d1 <- S d1 (rounded up),
 * which md_list_rows reports as after md_scale_cell; its scalars m0, m1 multiply s0, s1 on a handle that sees both calls,
 * and a handle that sees md_scale_cell alone gets the doubles it always got.  *rows_kept = 0 and both lists retire (the next
 * evaluation builds in the new cell with the full skin) when skin_eff falls below two thirds of the configured skin, a
 * particle lies beyond skin_eff / 2 of its mapped x0 (measured in the same pass), the rows are not the tiled two-level kind
 * (user potential, skin 0, rows that do not fit LDS; the frame is simply mapped), or the call changes the cell between
 * diagonal and general (kernels that read the live rows branch on that: the first shear of an orthorhombic box costs one
 * build).  The inner rows alone are dropped by the corresponding inner conditions.  Grids, capacities, md_rdf_ / md_mpc_,
 * md_hess_ / md_elas_: as md_scale_cell.  rows_kept may be NULL.  Waits.
 * Refused, with the handle exactly as before: md_scale_cell's refusals, and F or G not finite, det F <= 0.
 * md_deform_state (read-only): m0[9], m1[9] = M0, M1 as row-major 3 x 3 (identity when nothing was mapped since the build /
 * prune, or without valid rows; md_scale_cell's factors included), sig[4] = s0, S0, s1, S1 with S0 >= sigma_max(M0),
 * S1 >= sigma_max(M1).  Any of the three may be NULL.                                                                     */
int md_deform_cell(md_ctx *ctx, const double *F, const double *G, int *rows_kept);
int md_deform_state(md_ctx *ctx, double *m0, double *m1, double *sig);

/* Library build info: returns e.g. "mdhip 0.1 gfx950". */
const char *md_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MDHIP_H */
