// mdhip.hip -- host side of libmdhip.so: device-resident state, list (re)builds, the step
// loop and the extern "C" boundary declared in include/mdhip.h.
//
// Reference call stack this replaces: run_simulation! (src/simulation.jl:88-108) ->
// integrate_half! / reset_output! / CellListMap.map_pairwise! / integrate_second_half! /
// ensemble_step!.  See md_kernels.hpp for the kernels and DESIGN.md for the data layout.
#include <cstring>
#include <cstdlib>
#include <unistd.h>

#include "md_kernels.hpp"
#include "md_domain.hpp"
#include "md_rdf.hpp"
#include "md_dyn.hpp"
#include "md_sq.hpp"
#include "md_stress.hpp"
#include "md_boo.hpp"
#include "md_mpc.hpp"
#include "md_cluster.hpp"
#include "md_cage.hpp"
#include "md_chi4.hpp"
#include "md_cur.hpp"
#include "md_listrows.hpp"
#include "md_swap.hpp"
#include "md_hess.hpp"
#include "md_elas.hpp"
#include "md_cell.hpp"
#include "md_baro.hpp"
#include "md_deform.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mdhip.h"
#include "md_rtc.hpp"
#include "md_rccl.hpp"

static RcclApi g_rccl;
static const bool g_dom_group_flag = [] { const char *e = getenv("MDHIP_DOM_GROUP_FLAG"); return e && e[0] == '1'; }();

namespace {

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIPCHK(expr)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            char buf_[512];                                                                                 \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,    \
                     __LINE__);                                                                             \
            throw HipError(buf_);                                                                           \
        }                                                                                                   \
    } while (0)

template <class T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
    void alloc(size_t count)
    {
        release();
        if (count == 0) count = 1;
        HIPCHK(hipMalloc((void **)&p, count * sizeof(T)));
        n = count;
    }
    hipError_t try_alloc(size_t count) // alloc that reports instead of throwing; the buffer stays empty on failure
    {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e == hipSuccess)
            n = count;
        else
            p = nullptr;
        return e;
    }
    void ensure(size_t count)
    {
        if (count > n) alloc(count + count / 4 + 16);
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DBuf() { release(); }
};

// A sampler's large storage (md_dyn / md_chi4 origin slots, the md_cage table), `bytes` in all, described by `what`: the
// buffers are released, then allocated in order (one of count 0 stays empty).  The first failure -- or `bytes` above the
// value of the environment variable `limit_env`, a debug switch that refuses as if the device had run out of memory, so
// the message can be checked at a test size -- releases them all, clears the sticky error and throws.
template <class... B>
void alloc_or_refuse(const char *who, const char *limit_env, size_t bytes, const char *what, std::pair<B *, size_t>... bufs)
{
    (bufs.first->release(), ...);
    const char *lim = getenv(limit_env);
    hipError_t e = hipSuccess;
    if (lim && bytes > (size_t)strtoull(lim, nullptr, 10))
        e = hipErrorOutOfMemory;
    else
        (void)(... && (bufs.second == 0 || (e = bufs.first->try_alloc(bufs.second)) == hipSuccess));
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    (bufs.first->release(), ...);
    char b[400];
    snprintf(b, sizeof b, "%s: cannot allocate %zu bytes for %s: %s", who, bytes, what, hipGetErrorString(e));
    throw HipError(b);
}

// The origin slots and lag rows of a time-correlation sampler (md_dyn, md_sq, md_cage, md_chi4), on the host
struct SlotRows {
    int nslots = 0, nrows = 0;
    std::vector<char> filled;      // nslots: the slot holds an origin
    std::vector<int64_t> nsamples; // nrows: the (slot, row) pairs sampled into the row since setup / reset
    void init(int ns, int nr)
    {
        nslots = ns;
        nrows = nr;
        filled.assign(ns, 0);
        nsamples.assign(nr, 0);
    }
    void check_slot(const char *who, int slot) const // an origin store's target
    {
        if (slot >= 0 && slot < nslots) return;
        char b[160];
        snprintf(b, sizeof b, "%s: slot %d is out of range 0..%d", who, slot, nslots - 1);
        throw HipError(b);
    }
    void check_origin(const char *who, int slot) const // the origin store of a sample call (md_sq, md_cur): -1 = none
    {
        if (slot >= -1 && slot < nslots) return;
        char b[200];
        snprintf(b, sizeof b, "%s: origin slot %d is out of range -1..%d", who, slot, nslots - 1);
        throw HipError(b);
    }
    // The (slot, row) pairs of one sample call: every slot holds an origin, every row exists.
    void check_batch(const char *who, const int32_t *slots, const int32_t *rows, int count, const char *empty_hint) const
    {
        char b[200];
        if (count < 0) {
            snprintf(b, sizeof b, "%s: count must be >= 0, got %d", who, count);
            throw HipError(b);
        }
        if (count > 0 && (!slots || !rows)) throw HipError(std::string(who) + ": slots / rows is null");
        for (int i = 0; i < count; ++i) {
            check_slot(who, slots[i]);
            if (rows[i] < 0 || rows[i] >= nrows) {
                snprintf(b, sizeof b, "%s: row %d is out of range 0..%d", who, (int)rows[i], nrows - 1);
                throw HipError(b);
            }
            if (!filled[slots[i]]) {
                snprintf(b, sizeof b, "%s: slot %d is empty (%s)", who, (int)slots[i], empty_hint);
                throw HipError(b);
            }
        }
    }
    void count_rows(const int32_t *rows, int count)
    {
        for (int i = 0; i < count; ++i) ++nsamples[rows[i]];
    }
    void clear_counts() { std::fill(nsamples.begin(), nsamples.end(), (int64_t)0); }
    void read_counts(int64_t *out) const
    {
        if (out) std::copy(nsamples.begin(), nsamples.end(), out);
    }
};

inline int blocks_of(int64_t n, int per) { return (int)((n + per - 1) / per); }

// What mode_walk (md_sq.hpp) needs of a wave-vector sampler (md_sq, md_chi4, md_cur): the vectors, the particle blocks
// and the block partials
struct ModeSet {
    int nvec = 0, nvec_pad = 0, nblk = 0;
    DBuf<double> nd, part;         // nvec_pad x 3 wave vectors as doubles; (vector, accumulator, block)
    // The nv x dim integer vectors as the table the mode kernels read -- doubles, 3 per vector, padded with zero vectors
    // to whole md_sq tiles (none when nv == 0) -- and the partials of n particles, npv accumulators per vector.  Waits:
    // the table is a host vector.
    void init(const int32_t *nvecs, int nv, int dim, int64_t n, int npv, hipStream_t st)
    {
        nvec = nv;
        nvec_pad = (nv + MD_SQ_TILE - 1) / MD_SQ_TILE * MD_SQ_TILE;
        nblk = blocks_of(n, MD_SQ_BLOCK * MD_SQ_PPT);
        std::vector<double> t((size_t)nvec_pad * 3, 0.0);
        for (int v = 0; v < nv; ++v)
            for (int c = 0; c < dim; ++c) t[(size_t)v * 3 + c] = (double)nvecs[(size_t)v * dim + c];
        nd.alloc(t.size());
        part.alloc((size_t)nvec_pad * npv * std::max(nblk, 1));
        if (nv) HIPCHK(hipMemcpyAsync(nd.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
};

struct StateBufs {
    DBuf<double4> pos;
    DBuf<double> v[3], f[3], x0[3];
    DBuf<int32_t> img[3], id;
};

inline int ceil_log2(uint64_t v)
{
    int b = 0;
    while ((1ull << b) < v) ++b;
    return b;
}

std::string g_create_error;

} // namespace

struct md_ctx {
    int dim = 3;
    int64_t n = 0;        // particles this handle owns right now
    int64_t ncap = 0;     // capacity of the per-owned arrays (== n for a single-GPU handle)
    int64_t n_global = 0; // particles in the whole system (id range)
    int64_t src_count = 0; // live entries of pos/id in the current buffer (sources of the next build)
    // slab decomposition (md_create_domain); off for a single-GPU handle
    struct Domain {
        bool on = false;
        int rank = 0, nranks = 1;
        double xlo = 0.0, xhi = 0.0;
        int64_t n_old = 0, n_arr = 0, n_xh = 0; // sources of the build in progress
        int64_t nsend_mig[2] = {0, 0}, nsend_halo[2] = {0, 0}, nrecv_halo[2] = {0, 0};
        DBuf<int32_t> alive, counters, hs_src[2], send_slot[2], xh_slot;
        DBuf<double> sbuf[2], rbuf[2];
        double *ext_send[2] = {nullptr, nullptr}, *ext_recv[2] = {nullptr, nullptr}; // caller-owned step buffers
        int64_t ext_cap = 0;
        // asynchronous stepping (md_dom_async_*): caller-owned device words the caller all-reduces between the
        // phases of a step
        int32_t *flag_dev = nullptr; // [1] first violating step (MIN-reduced)
        double *kuw_dev = nullptr;   // [3] K, U, W partial sums of this rank (SUM-reduced)
        bool a_nvt = false;
        double a_nf = 0.0, a_term1 = 0.0;
        int64_t w_nsteps = 0, w_b0 = 0, w_prune_interval = 0; // the window being enqueued
        bool w_scale_from_sums = false; // NVT: the next kick-drift forms the scale from kuw_dev (step_c was skipped)
        std::vector<int> w_prune_steps;
        // native transport (md_dom_comm_init): RCCL called by the library on the handle's stream
        ncclComm_t comm = nullptr;
        bool prune_enabled = false; // inner rows on a slab handle: the caller plans the (globally identical) schedule
        DBuf<int32_t> own_flag;
        DBuf<int64_t> cnt_dev; // list build: record counts to / from the neighbours
        // fused window: boundary tiles (x-halo in their staged set, or owners of send-list particles) and the rest
        DBuf<int32_t> tile_flag, tiles_b, tiles_i;
        int n_tiles_b = 0, n_tiles_i = 0;
        hipStream_t stream_i = nullptr; // the interior tiles' stream
        hipEvent_t ev_go = nullptr, ev_int = nullptr;
        DBuf<double> own_kuw;
        // a fused window refreshes the x-halo particles' state RECORDS every step, not their pos[] entries: until the
        // next list build (or a classic step's coordinate exchange) md_dom_forces would read stale neighbour coordinates
        bool xhalo_pos_stale = false;
        // direct peer exchange (md_domain.hpp): this rank's mailbox, its peers' mailboxes as mapped here
        struct P2p {
            bool on = false;
            char *mail = nullptr;
            int64_t cap = 0; // records per receive plane of THIS rank's mailbox
            char *peer[MD_P2P_MAXR] = {};
            bool opened[MD_P2P_MAXR] = {};
            int64_t peer_cap[MD_P2P_MAXR] = {};
            unsigned long long seq = 0; // exchanges so far (all ranks count the same ones)
            unsigned *done = nullptr;
            long long timeout = 0;
            bool window = false; // the window being enqueued uses it (agreed by all ranks)
        } p2p;
    } dom;
    double L[3] = {1, 1, 1};
    // general (triclinic) unit cell: A = the cell matrix (row-major 3 x 3, columns = lattice vectors), Ainv its inverse,
    // perp[c] = distance between the faces of lattice direction c (1 / |row c of Ainv|), volume = |det A|.
    // tric == 0 (diagonal matrix): A = diag(L), perp = L.
    int tric = 0;
    double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Ainv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double perp[3] = {1, 1, 1};
    double volume = 1.0;
    double rc = 0.0;       // list cutoff (CellListMap's cutoff)
    double skin_req = 0.6; // requested skin.  Measured best for LJ r_c=2.5 at N=2^20: 0.6 with inner rows
                           // (inner skin 0.16), 0.4 without them
    double skin = 0.0;     // effective skin
    double rl = 0.0;       // rc + skin
    int pot_kind = POT_LJ;
    PotParams pp{};
    RtcModule *rtc = nullptr; // run-time compiled kernels of a user potential (POT_CUSTOM)
    bool uniform_sigma = true;
    double sigma_u = 1.0;
    double sigma_max = 1.0; // the largest diameter uploaded (pos[].w starts at 1)
    int device = 0;
    hipStream_t stream = nullptr;     // the stream every kernel of the handle runs on
    hipStream_t own_stream = nullptr; // the one created with the handle (stream may be the caller's: md_set_stream)

    int64_t cap = 0;  // extended capacity: owned + ghosts (sentinel lives at index cap)
    int64_t next = 0; // owned + ghosts of the last build
    int64_t nghost = 0;
    StateBufs sb[2];
    int cur = 0;
    BoxGrid grid{};
    int ncell_ext = 0;

    DBuf<int32_t> nimg, img_off, newslot, gsrc, gowner, cell_start, cell_end, nneigh, nmax_tile;
    DBuf<uint32_t> gcode, vals_in, vals_out, nlist, halo;
    DBuf<uint16_t> nlist16;
    DBuf<int32_t> halo_count;
    DBuf<long long> dbg_stamps;
    int hcap = 4096;       // halo slots per tile in global memory
    int hstride = 0;       // LDS plane stride (doubles) of the last build
    size_t tile_lds = 0;   // dynamic LDS bytes of the tiled force kernel
    bool use_tiles = false;
    int tile_rs = 24;
    bool allow_tiles = true;
    bool allow_fused_build = true;
    bool allow_own_first = true;  // MDHIP_NO_OWN_FIRST=1: k_build_tile numbers the halo cell by cell throughout
    bool own_first = false;       // halo slots [0, 256) of every tile are its own particles (rows of the last build came from k_build_tile)
    bool own_first_staged = false; // the last step launch staged the own records from registers
    bool have_nlist32 = false; // the 32-bit global-index rows exist for the current build
    DBuf<uint64_t> keys_in, keys_out;
    DBuf<char> sort_tmp, scan_tmp;
    int maxn = 0;
    int64_t ntiles = 0;

    DBuf<double> partials;
    DBuf<double> fire_part;      // FIRE: per-block sums of |f|^2, v.f, |v|^2
    DBuf<FireState> fire_state;
    DBuf<double> brown_acc;      // Brownian: {sum of sampled virials, number of samples}
    int nblk = 0;
    DBuf<Scalars> scal;
    DBuf<double> d_kt, d_r1, d_r2;

    DBuf<double> io_x, io_v, io_f, io_d;
    DBuf<int32_t> io_i;
    // asynchronous frame export (md_snapshot_begin / md_snapshot_end): device staging of its own, pinned host buffers,
    // a copy stream, and the event the host waits on
    DBuf<double> snap_x;
    DBuf<int32_t> snap_i;
    double *pin_x = nullptr;
    int32_t *pin_i = nullptr;
    size_t pin_n = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_snap_ready = nullptr, ev_snap_copied = nullptr;
    bool snap_pending = false;

    bool list_valid = false;
    int64_t steps_since_build = 0;
    int64_t target_interval = 8;
    // dynamic pruning of the rows (single-GPU handles with a skin): inner rows used by the force kernel
    double inner_skin_req = 0.16; // prune step every ~10 steps at dt=0.001, kT~1.5
    double inner_skin = 0.0;
    bool virtual_ghosts = false; // halo entries of ghosts are (owner | shift code << 26): no per-step ghost refresh
    bool inner_valid = false; // the inner rows exist and the force kernel uses them
    bool prune_on = false;    // this build supports inner rows (tiled path, skin > inner skin > 0, single GPU)
    DBuf<double> x1[3];
    DBuf<uint16_t> nlist16_in;
    DBuf<int32_t> nmax_tile_in;
    int64_t steps_since_prune = 0;
    // fused step loop (k_step_tile): ping-pong state records; `fz_a` = the buffer set that holds the latest complete
    // step: records rec[fz_a], forces sb[cur ^ fz_a].f, positions sb[cur ^ fz_a].pos  (set 0 is the canonical state)
    DBuf<double2> rec[2];
    // inner halo of the fused loop: per tile, the outer-halo records within (cutoff + inner skin) of the tile's own
    // particles at the last prune step; ordinary steps stage only those
    DBuf<uint32_t> halo_in;
    DBuf<int32_t> halo_in_count;
    int hcap_in = 0;
    size_t tile_lds_in = 0;
    bool allow_inner_halo = true;
    bool inner_halo_live = false; // the current inner rows index the inner halo image (written by a fused prune step)
    int fz_a = 0;
    bool allow_fused = true;
    double d1_rate = 0.0;       // growth per step of the largest displacement since a reference (measured)
    bool rate_known = false;
    double safety = 0.97;       // fraction of the validity radii the plan uses
    int64_t st_prunes = 0;
    // md_scale_cell (md_baro.hpp): the product of its factors since the outer build (m0) and since the last prune (m1),
    // and whether there was any -- a list that was never scaled uses skin and inner_skin as they are, not times 1.0.
    // grid_stale: the cell changed under live rows; the cell grid and the capacities follow at the next build.
    double m0 = 1.0, m1 = 1.0;
    bool scaled0 = false, scaled1 = false;
    bool grid_stale = false;
    DBuf<unsigned long long> scale_dmax; // what the last md_scale_cell's pass reported (md_baro.hpp, MD_SCALE_NOUT words)
    // md_deform_cell (md_deform.hpp): the product of its F's since the outer build (Md0) and since the
    // last prune (Md1), row-major 3 x 3, and rigorous bounds on their singular values: ds <= sigma_min, dS >= sigma_max.
    // A list that was never deformed uses none of them (deformed0 / deformed1 false): md_scale_cell's doubles as they were.
    double Md0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Md1[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double ds0 = 1.0, dS0 = 1.0, ds1 = 1.0, dS1 = 1.0;
    bool deformed0 = false, deformed1 = false;

    // stats / profiling
    int64_t st_steps = 0, st_rebuilds = 0, st_viol = 0;
    bool prof = false;
    int prof_stride = 1;          // time every prof_stride-th launch of each kind (event records cost ~4 us each)
    int64_t prof_seen[2] = {0, 0};
    bool prof_open = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
    size_t prof_used = 0;
    double prof_ms_acc = 0.0;
    int64_t prof_launch_acc = 0;
    std::vector<int> prof_tag;          // 0: force kernel, 1: kick-drift kernel
    double prof_kd_ms_acc = 0.0;
    int64_t prof_kd_launch_acc = 0;
    int64_t prof_prune_acc = 0;   // timed force/step launches that were prune steps
    double prof_prune_ms_acc = 0.0;
    double prof_rebuild_ms_acc = 0.0;
    int64_t prof_rebuild_acc = 0;
    bool prof_cur_prune = false;  // the launch being timed is a prune step
    bool last_run_fused = false;
    // launch_step over a subset of the tiles (slab windows: boundary tiles ahead of the interior ones)
    struct StepPart {
        const int32_t *list = nullptr;
        int count = 0;
        hipStream_t stream = nullptr;
        bool last = true; // the launch that completes the step: host-side bookkeeping happens here
    } part;

    // radial distribution function (md_rdf_*): a grid of its own, scratch for the sort, the histogram
    struct Rdf {
        bool on = false;
        double r_max = 0.0;
        int nbins = 0;
        RdfGrid grid{};
        int64_t nsamples = 0;
        DBuf<double> e2;                  // nbins + 1 squared bin edges
        DBuf<unsigned long long> hist;    // nbins
        DBuf<double4> wrec, srec;         // n: wrapped records {x, y, z, id}, in slot order / in cell order
        DBuf<uint32_t> keys_in, keys_out, vals_in, vals_out;
        DBuf<int32_t> cell_start, cell_end, work;
        DBuf<char> sort_tmp;
    } rdf;

    // self dynamics (md_dyn_*): the slot / row bookkeeping, origin frames in slots, the current frame, block partials,
    // per-row sums and histograms
    struct Dyn {
        bool on = false;
        int nq = 0, nbins = 0;
        double r_max = 0.0;
        std::vector<double> q;
        SlotRows sr;
        DBuf<double> ox;                  // nslots frames of n x dim wrapped coordinates, in particle-id order
        DBuf<int32_t> oi;                 // nslots frames of n x dim image counts
        DBuf<double> cx, part, sums, e2;  // current frame; block partials of one batch; nrows x (2 + nq); nbins + 1
        DBuf<int32_t> ci;
        DBuf<unsigned long long> hist;    // nrows x nbins
    } dyn;

    // density modes (md_sq_*): the slot / row bookkeeping (both may be empty), the wave vectors, the current frame and its
    // fractional coordinates, block partials, rho of the last sampled frame, the static and the correlation accumulators,
    // rho of the stored origins
    struct Sq : ModeSet {
        bool on = false;
        bool sampled = false;             // rho holds a frame
        int64_t nstatic = 0;
        SlotRows sr;
        DBuf<double> cx, fr, rho, s2, corr, org; // frame; f per axis; 2 nvec; nvec; nrows x nvec; nslots x nvec x 2
        DBuf<int32_t> ci;
    } sq;

    // pressure tensor (md_stress_*): block partials, the last frame's tensor, the running sums, the channel ring and the
    // lag products
    struct Stress {
        bool on = false;
        bool sampled = false;             // last holds a frame
        int nlags = 0;
        int64_t nsamples = 0;             // since setup / reset: the next sample's number m
        DBuf<double> part, last, sums, ring, corr; // 2 nc x nblk; 2 nc; 2 nc; nlags x nc; nlags x nc
    } stress;

    // bond-orientational order (md_boo_*): per-slot q_lm (component-major), its norm, n_i, q, qbar and c_i of the last
    // frame and that frame's slot -> particle-id permutation (the handle's own changes with every list build and upload);
    // block partials; the running sums, the series; the four histograms in one buffer
    struct Boo {
        bool on = false;
        bool sampled = false;             // the per-slot arrays and last hold a frame
        int order = 6, nm = 7, nbins = 0, min_conn = 0;
        double rn = 0.0, rn2 = 0.0, threshold = 0.0;
        int64_t nseries = 0;
        int64_t nsamples = 0;             // since setup / reset: the next sample's number m
        BooCoef coef{};
        DBuf<double> qlm, norm, q, qbar, part, sum_fr, series, io_d; // 2 nm x n; n; n; n; (7 + 2 nm) x nblk; 8; nseries x 8
        DBuf<int32_t> nnb, nconn, ids, io_i;
        DBuf<unsigned long long> hist;    // 2 nbins + 2 x 33
        size_t nhist() const { return (size_t)2 * nbins + 2 * (MD_BOO_NCLAMP + 1); }
    } boo;

    // clusters (md_cluster_*): the union-find forest, the per-slot member flag, root, and per-root size and smallest id of
    // the last frame with that frame's slot -> particle-id permutation; the by-id solid mask; block partials; the running
    // sums, the series and the size histogram -- all integers
    struct Cluster {
        bool on = false;
        bool sampled = false;             // root / count / minid / ids hold a frame
        int members = 0, max_size = 0;
        double rb = 0.0, rb2 = 0.0;
        int64_t nseries = 0;
        int64_t nsamples = 0;             // since setup / reset: the next sample's number m
        DBuf<uint32_t> parent, root;      // n; n
        DBuf<int32_t> count, minid, ids, io_i; // n; n; n; 2 n
        DBuf<unsigned char> mem, mask;    // n (by slot); n (by particle id, SOLID only)
        DBuf<unsigned long long> part, deg, hist; // 6 x nblk (256-slot blocks); the hook kernel's blocks; max_size + 1
        DBuf<long long> sum_fr, series;   // 8; nseries x 8
    } cluster;

    // cage-relative dynamics and bond breaking (md_cage_*): the slot / row bookkeeping; per origin slot the frame, n_i,
    // sigma and -- the table -- the entry lists (id_j, del_ij), all by particle id; the current frame, the displacements of
    // one batch, block partials; per-row sums, counts and histograms; the last sample's per-particle arrays; the
    // dropped-hit counter
    struct Cage {
        bool on = false;
        bool sampled = false;             // l_nnb / l_broken / l_d2 hold a sample
        int nq = 0, max_neigh = 0, scaled = 0;
        double r_neigh = 0.0, r_break = 0.0;
        std::vector<double> q;
        SlotRows sr;
        DBuf<int32_t> nid;                // the table: nslots x max_neigh x n ids ...
        DBuf<double> del;                 // ... and nslots x max_neigh x dim x n bond components
        DBuf<double> ox, cx, sig, disp, part, sums, l_d2; // nslots frames; frame; nslots x n; batch x dim x n; ...; nrows x (2 + nq); n
        DBuf<int32_t> oi, ci, nnb, l_nnb, l_broken;       // nslots frames; frame; nslots x n; n; n
        DBuf<unsigned long long> counts, hist, overflow;  // nrows x 3; nrows x 33; 1
    } cage;

    // four-point dynamics (md_chi4_*): the slot / row bookkeeping; per origin slot the frame and -- with vectors -- its
    // fractional coordinates; the current frame; the mask, the block partials, Q and W of the sample in flight / the last
    // one; the rows
    struct Chi4 : ModeSet {
        bool on = false;
        bool sampled = false;             // mask / qlast / wlast hold a sample
        int nwords = 0;
        double a = 0.0, a2 = 0.0;
        SlotRows sr;                      // (sr.nsamples: the host's count, behind the sum_q2 overflow guard)
        DBuf<double> ox;                  // nslots frames of n x dim wrapped coordinates, in particle-id order
        DBuf<int32_t> oi;                 // nslots frames of n x dim image counts
        DBuf<double> of;                  // nslots frames of dim x n fractional coordinates, one array per axis (nvec > 0)
        DBuf<double> cx, wlast, s4;       // frame; 2 nvec; nrows x nvec
        DBuf<int32_t> ci;
        DBuf<unsigned long long> mask, qcur; // nwords; 1
        DBuf<long long> qlast, irow;      // 1; nrows x MD_CHI4_NROW
    } chi4;

    // currents and the VACF (md_cur_*): the slot / row bookkeeping (both may be empty); the wave vectors and their unit
    // directions; the current frame, its f and v per axis; block partials, j of the last sampled frame, the static and
    // the correlation accumulators, j of the stored origins; with vacf the origins' velocity frames, the pair partials
    // and z (nrows lag rows, then the equal-time row)
    struct Cur : ModeSet {
        bool on = false;
        bool vacf = false;
        int zblk = 0;
        bool sampled = false;             // jl holds a frame
        int64_t nstatic = 0;
        SlotRows sr;
        DBuf<double> e;                   // nvec x dim unit directions
        DBuf<double> cx, cv, fr, va;      // frame x, v (n x dim); f and v per axis
        DBuf<int32_t> ci;
        DBuf<double> jl, s_tot, s_long, c_tot, c_long, org; // nvec x dim x 2; nvec; nvec; nrows x nvec (2); nslots x nvec x dim x 2
        DBuf<double> ov, zpart, z;        // nslots frames of n x dim velocities; batch x zblk; nrows + 1
    } current;

    // marked pair correlations (md_mpc_*): a grid and sort scratch of its own (not the rdf sampler's: both can be set up
    // at once), the marks by particle id (user source) and in sorted order, the inverse of the bond-order frame's
    // permutation (boo source); the per-sample words, the last sample, the accumulators, the sticky error bits
    struct Mpc {
        bool on = false;
        bool sampled = false;             // last_* hold a sample
        bool have_marks = false;          // user source: md_mpc_marks has been called
        int source = 0, nc = 0, nbins = 0;
        double r_max = 0.0, tmax = 0.0;
        MpcWeights w{};
        RdfGrid grid{};
        int64_t nsamples = 0;
        DBuf<double> e2, marks, smarks;   // nbins + 1; n x nc by id; n x nc in sorted order
        DBuf<int32_t> inv;                // n
        DBuf<double4> wrec, srec;
        DBuf<uint32_t> keys_in, keys_out, vals_in, vals_out;
        DBuf<int32_t> cell_start, cell_end, work, range_error;
        DBuf<char> sort_tmp;
        DBuf<unsigned long long> cur_cnt, last_cnt, acc_cnt; // nbins each
        DBuf<long long> cur_sum, last_sum, self;  // nbins; nbins; {cur, last}
        DBuf<double> acc_sum, acc_self;   // nbins; 1
    } mpc;

    // swap Monte Carlo (md_swap_*): the claims, the live keys, the compact member list and the per-entry results of the
    // round in flight; partner / status / dU of the last round by particle id; the counters and the running sum of the
    // accepted dU of one md_swap_rounds call
    struct Swap {
        bool on = false;
        bool ran = false;                 // partner / status / du hold a round
        double fraction = 0.0, max_diff = 0.0;
        uint64_t seed = 0;
        uint32_t thr = 0;
        DBuf<unsigned long long> claim, livekey, counts; // n; n; MD_SWAP_NCOUNT
        DBuf<int32_t> partner, status, entry, members, blocked, nmember, inv; // n; n; n; 2 n + 4; n + 2; 1; n
        DBuf<double> half, du, part, du_acc;             // n + 2; n; blocks; 1
    } swap;

    // Hessian of the pair energy (md_hess_*): `frozen` = the operator belongs to the frame and the rows the handle holds
    // right now; everything that moves particles, changes diameters or the potential, or rebuilds the list clears it.
    // Block staging (xs, ys: n x 8 D, slot-major), the diagonal blocks, and the Lanczos storage: the basis (kcap vectors of
    // n D), the work vector, chunk partials, pass coefficients, alpha and beta, the Ritz coefficients.
    struct Hess {
        bool frozen = false;
        DBuf<double> xs, ys, diag, host_io;
        DBuf<double> basis, w, part, coef, alpha, beta, S;
        int kcap = 0;      // basis vectors allocated
        int ksteps = 0;    // basis vectors the last md_hess_lanczos filled (0: none, or of an older frame)
        uint64_t epoch = 0; // md_hess_setup calls so far: names the operator to whatever derives state from it (md_elas_*)
    } hess;

    // Elastic moduli (md_elas_*): `epoch` = the md_hess_setup whose operator the affine pass walked (0: none); whatever
    // clears hess.frozen forces a new md_hess_setup and with it a new epoch, so there is no second flag to clear.  The
    // affine force field xi and the solver's vectors (n x M D each, slot-major, M = hess_block(nc)), which particles have
    // a bond, the block / chunk partials, the finished sums and the solver's scalars.
    struct Elas {
        uint64_t epoch = 0;
        DBuf<double> xi, x, r, p, hp, part, sums, mean, out, host_io;
        DBuf<int32_t> bonded;
        DBuf<ElasScal> sc;
    } elas;

    // Non-affine displacement since a mark (md_nonaffine_*): the mark by particle id -- fractional coordinates and image
    // counts, kept apart so that the image difference is exact -- the per-particle u (when asked for), block partials of
    // the sums, per-block maximum bits and ids, the global maximum's bits, the finished sums.
    struct Naff {
        bool marked = false;
        DBuf<double> frac, u, part, out;  // n x dim; n x dim; MD_NAFF_NSUM x nblk; 8
        DBuf<int32_t> img, pid;           // n x dim; nblk
        DBuf<unsigned long long> pmax, gmax; // nblk; 1
        DBuf<int> range_error;            // md_set_cell, MD_CELL_LATTICE: an image count would leave int32
    } naff;

    std::string err;
    // A failure inside a fused step loop (between fused_enter and fused_leave) leaves the live state in the step
    // records and whichever buffer set the ping-pong points at: pos / v / f are stale.  Every entry that reads the state
    // refuses to go on until a full md_upload (x, v and f) replaces it.
    bool state_invalid = false;

    DevState dev(int which)
    {
        DevState s{};
        StateBufs &b = sb[which];
        s.pos = b.pos.p;
        for (int c = 0; c < 3; ++c) {
            s.v[c] = b.v[c].p;
            s.f[c] = b.f[c].p;
            s.img[c] = b.img[c].p;
            s.x0[c] = b.x0[c].p;
            s.x1[c] = (inner_valid && x1[c].p) ? x1[c].p : b.x0[c].p;
        }
        s.id = b.id.p;
        for (int c = 0; c < 3; ++c) s.boxL[c] = c < dim ? L[c] : 0.0;
        s.tric = tric;
        for (int c = 0; c < 9; ++c) s.cellA[c] = A[c];
        return s;
    }
};

namespace {

inline int nblocks(int64_t n) { return (int)((n + MD_BLOCK - 1) / MD_BLOCK); }

// What the rows in use still allow.  Rows built at radius rl are, after isotropic scales of the
// frame by a total of m0, complete about the scaled x0 to m0 * rl; the inner rows likewise to m1 * (cutoff + inner skin)
// about the scaled x1.  The cutoff does not scale, so the skins left are these.  Without a scale since the build (the
// prune) they are the configured doubles themselves.
// After md_deform_cell (section 27) the factor is a lower bound on the smallest singular value of the accumulated map: the
// scalar of md_scale_cell times ds0 (ds1).  A list that was only ever scaled takes the first branch: the doubles of section 26.
inline double rl_eff(const md_ctx *c)
{
    if (c->deformed0) return (c->m0 * c->ds0) * c->rl;
    return c->scaled0 ? c->m0 * c->rl : c->rl;
}
inline double skin_eff(const md_ctx *c)
{
    if (c->deformed0) return (c->m0 * c->ds0) * c->rl - c->rc;
    return c->scaled0 ? c->m0 * c->rl - c->rc : c->skin;
}
inline double inner_eff(const md_ctx *c)
{
    if (c->deformed1) return (c->m1 * c->ds1) * (c->rc + c->inner_skin) - c->rc;
    return c->scaled1 ? c->m1 * (c->rc + c->inner_skin) - c->rc : c->inner_skin;
}
inline void deform_reset1(md_ctx *c)
{
    for (int i = 0; i < 9; ++i) c->Md1[i] = (i % 4 == 0) ? 1.0 : 0.0;
    c->ds1 = c->dS1 = 1.0;
    c->deformed1 = false;
}
inline void deform_reset0(md_ctx *c)
{
    for (int i = 0; i < 9; ++i) c->Md0[i] = (i % 4 == 0) ? 1.0 : 0.0;
    c->ds0 = c->dS0 = 1.0;
    c->deformed0 = false;
}

__global__ void k_init_state(int n, int64_t cap, DevState s, int dim)
{
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > cap) return;
    bool sent = (k == cap);
    double sp = sent ? MD_SENTINEL_POS : 0.0;
    s.pos[k] = make_double4(sp, sp, dim == 3 ? sp : 0.0, 1.0);
    s.id[k] = sent ? -1 : (k < n ? (int32_t)k : 0);
    if (k < n)
        for (int c = 0; c < dim; ++c) {
            s.v[c][k] = 0.0;
            s.f[c][k] = 0.0;
            s.img[c][k] = 0;
            s.x0[c][k] = 0.0;
        }
}

__global__ void k_reset_flags(Scalars *sc) { reset_flags(sc); }

__global__ void k_reset_disp0(Scalars *sc) { sc->max_disp2_bits = 0ull; }
__global__ void k_clear_halo_overflow(Scalars *sc) { sc->halo_overflow = 0; }

// before a prune step: the displacement maximum since the build is recomputed by that step
// (skipped, like the step itself, when an earlier step of the window recorded a violation)
__global__ void k_reset_d1(Scalars *sc, int step)
{
    if (step >= 0 && sc->first_viol <= step) return;
    sc->d1max2_bits = 0ull;
}

void alloc_state(md_ctx *c, int which, int64_t cap)
{
    StateBufs &b = c->sb[which];
    b.pos.alloc(cap + 1);
    for (int d = 0; d < c->dim; ++d) {
        b.v[d].alloc(c->ncap);
        b.f[d].alloc(c->ncap);
        b.img[d].alloc(c->ncap);
        b.x0[d].alloc(c->ncap);
    }
    b.id.alloc(cap + 1);
}

// The unit cell handed to md_create: classification, inverse and face distances.  The inverse is formed exactly as the
// oracle forms it (oracle/md_oracle.c oracle_set_cell: cofactors over the determinant, no fma), so that both sides wrap
// with the same U^-1 -- the reference's `unitcell \\ x` (src/boundary.jl:9) solves by LU instead; the difference is a
// rounding in the fractional coordinate, which matters only for a particle within an ulp of a face.
struct CellGeom {
    int tric = 0;
    double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Ainv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double perp[3] = {1, 1, 1};
    double volume = 1.0;
};
const char *cell_geometry(int dim, const double *box, CellGeom &g)
{
#pragma clang fp contract(off)
    bool diag = true;
    for (int r = 0; r < dim; ++r)
        for (int c = 0; c < dim; ++c) {
            double v = box[c * dim + r];
            if (!std::isfinite(v)) return "md_create: unit cell entries must be finite";
            if (r != c && v != 0.0) diag = false;
            g.A[r * 3 + c] = v;
        }
    if (diag) {
        g.volume = 1.0;
        for (int c = 0; c < dim; ++c) {
            double v = g.A[c * 3 + c];
            if (!(v > 0.0)) return "md_create: box lengths must be positive";
            g.Ainv[c * 3 + c] = 1.0 / v;
            g.perp[c] = v;
            g.volume *= v;
        }
        g.tric = 0;
        return nullptr;
    }
    const double *U = g.A;
    double det;
    if (dim == 2) {
        det = U[0] * U[4] - U[1] * U[3];
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return "md_create: the unit cell matrix is singular";
        g.Ainv[0] = U[4] / det;
        g.Ainv[1] = -U[1] / det;
        g.Ainv[3] = -U[3] / det;
        g.Ainv[4] = U[0] / det;
    } else {
        double c00 = U[4] * U[8] - U[5] * U[7], c01 = U[5] * U[6] - U[3] * U[8], c02 = U[3] * U[7] - U[4] * U[6];
        det = (U[0] * c00 + U[1] * c01) + U[2] * c02;
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return "md_create: the unit cell matrix is singular";
        g.Ainv[0] = c00 / det;
        g.Ainv[1] = (U[2] * U[7] - U[1] * U[8]) / det;
        g.Ainv[2] = (U[1] * U[5] - U[2] * U[4]) / det;
        g.Ainv[3] = c01 / det;
        g.Ainv[4] = (U[0] * U[8] - U[2] * U[6]) / det;
        g.Ainv[5] = (U[2] * U[3] - U[0] * U[5]) / det;
        g.Ainv[6] = c02 / det;
        g.Ainv[7] = (U[1] * U[6] - U[0] * U[7]) / det;
        g.Ainv[8] = (U[0] * U[4] - U[1] * U[3]) / det;
    }
    for (int r = 0; r < dim; ++r) {
        double n2 = 0.0;
        for (int c = 0; c < dim; ++c) n2 += g.Ainv[r * 3 + c] * g.Ainv[r * 3 + c];
        g.perp[r] = 1.0 / std::sqrt(n2);
    }
    g.volume = std::fabs(det);
    g.tric = 1;
    return nullptr;
}

// (re)derive the cell grid from box, cutoff and skin
void configure_grid(md_ctx *c)
{
    // width of this handle's region per dimension (a slab handle owns [xlo, xhi) in x)
    // (general cell: the distance between opposite faces -- cells are cut in fractional coordinates, md_kernels.hpp cell_coords)
    double W[3] = {c->perp[0], c->perp[1], c->perp[2]};
    if (c->dom.on) W[0] = c->dom.xhi - c->dom.xlo;
    double lmin = 1e300;
    for (int d = 0; d < c->dim; ++d) {
        // a self-periodic dimension needs 3 cells (its two image layers must be distinct cells);
        // the decomposed one needs 2
        double need = (c->dom.on && d == 0) ? 2.0 : 3.0;
        lmin = std::min(lmin, W[d] / need);
    }
    if (lmin < c->rc) {
        char b[256];
        snprintf(b, sizeof b,
                 "box too small for the linked-cell build: need every box length (general cell: face distance) >= 3*list_cutoff (slab width >= "
                 "2*list_cutoff); got limit %g for list_cutoff=%g",
                 lmin, c->rc);
        throw HipError(b);
    }
    double skin = std::max(0.0, c->skin_req);
    double smax = lmin - c->rc;
    if (skin > smax) skin = std::max(0.0, smax * 0.999);
    c->skin = skin;
    c->rl = c->rc + skin;
    BoxGrid &g = c->grid;
    int64_t ncell = 1;
    for (int d = 0; d < 3; ++d) {
        g.lo[d] = 0.0;
        g.selfimg[d] = 1;
        if (d < c->dim) {
            g.L[d] = c->L[d];
            g.invL[d] = 1.0 / c->L[d];
            int kmin = (c->dom.on && d == 0) ? 2 : 3;
            int k = (int)std::floor(W[d] / c->rl);
            // guard against floor() landing one too high through rounding
            while (k > kmin && W[d] / k < c->rl) --k;
            if (k < kmin) k = kmin;
            g.nc[d] = k;
            g.ncx[d] = k + 2;
            g.inv_cell[d] = (double)k / W[d];
        } else {
            g.L[d] = 1.0;
            g.invL[d] = 1.0;
            g.nc[d] = 1;
            g.ncx[d] = 1;
            g.inv_cell[d] = 0.0;
        }
    }
    if (c->dom.on) {
        g.lo[0] = c->dom.xlo;
        g.selfimg[0] = 0;
    }
    g.tric = c->tric;
    for (int d = 0; d < 9; ++d) {
        g.A[d] = c->A[d];
        g.Ainv[d] = c->Ainv[d];
    }
    // brick-major cell numbering: balanced bricks of about 2x2x3 cells (4x3 in 2-D)
    int target[3] = {2, 2, 3};
    if (c->dim == 2) {
        target[0] = 4; target[1] = 3; target[2] = 1;
    }
    int64_t nint = 1, next_plain = 1;
    for (int d = 0; d < 3; ++d) {
        g.nb[d] = std::max(1, g.nc[d] / target[d]);
        g.bd[d] = (g.nc[d] + g.nb[d] - 1) / g.nb[d]; // largest brick along d
        nint *= (int64_t)g.nb[d] * g.bd[d];
        next_plain *= g.ncx[d];
    }
    ncell = nint + next_plain;
    g.n_int_cells = (int)nint;
    if (ncell > (1ll << 30)) throw HipError("cell grid too large");
    c->ncell_ext = (int)ncell;
    g.id_bits = std::max(1, ceil_log2((uint64_t)std::max<int64_t>(c->n_global, 2)));
    g.cell_bits = std::max(1, ceil_log2((uint64_t)ncell));
    c->cell_start.ensure(ncell + 1);
    c->cell_end.ensure(ncell + 1);
    c->list_valid = false;
    c->grid_stale = false;
}

// Smallest double t with sqrt(t) >= r (sqrt correctly rounded, as IEEE and Julia's sqrt are): the reference
// zeroes a pair iff sqrt(d2) >= r_cut (src/pairwise.jl:29, src/potentials.jl:67-69), i.e. iff d2 >= this
// threshold -- which is NOT r*r in general (sqrt(6.25 - 1 ulp) already rounds to 2.5).
double sqrt_ge_threshold(double r)
{
    if (!(r > 0.0) || !std::isfinite(r)) return 0.0; // (rejected by md_set_potential; never loop on it)
    double t = r * r;
    // r*r is within one ulp of the threshold: a handful of steps either way, bounded so that nothing can spin here
    for (int i = 0; i < 64 && t > 0.0 && std::sqrt(t) >= r; ++i) t = std::nextafter(t, 0.0);
    for (int i = 0; i < 64 && std::sqrt(t) < r; ++i) t = std::nextafter(t, INFINITY);
    return t;
}

void configure_potential(md_ctx *c)
{
    double c2_incl = c->rc * c->rc;
    double c2 = std::nextafter(c2_incl, INFINITY); // d2 < c2  <=>  d2 <= rc^2   (CellListMap's acceptance)
    if (c->pot_kind == POT_LJ || c->pot_kind == POT_LJ_MOD) {
        // r >= r_cut -> (0,0) with r = sqrt(d2): src/potentials.jl:67-69
        c2 = std::min(c2, sqrt_ge_threshold(c->pp.p[2]));
    }
    c->pp.c2 = c2;
    {
        uint64_t bits;
        memcpy(&bits, &c2, sizeof bits);
        c->pp.c2_k = (uint32_t)(bits >> 32) - 1u;
    }
    c->pp.sig_u = c->sigma_u;
    c->pp.sig2u = ((c->sigma_u + c->sigma_u) * 0.5) * ((c->sigma_u + c->sigma_u) * 0.5);
    c->pp.c48 = 48.0 * c->pp.p[0];
    c->pp.c24 = 24.0 * c->pp.p[0];
    c->pp.c4 = 4.0 * c->pp.p[0];
    double s6 = c->pp.sig2u * c->pp.sig2u * c->pp.sig2u;
    c->pp.ljA = c->pp.c48 * s6 * s6;
    c->pp.ljB = c->pp.c24 * s6;
}

void ensure_capacity(md_ctx *c, int64_t need_next)
{
    if (need_next <= c->cap) return;
    int64_t newcap = need_next + need_next / 8 + 1024;
    // grow both state buffers, preserving the current one's owned entries
    for (int w = 0; w < 2; ++w) {
        StateBufs &b = c->sb[w];
        DBuf<double4> np;
        np.alloc(newcap + 1);
        DBuf<int32_t> ni;
        ni.alloc(newcap + 1);
        if (w == c->cur) {
            int64_t keep = std::max(c->n, c->src_count);
            HIPCHK(hipMemcpyAsync(np.p, b.pos.p, sizeof(double4) * keep, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(ni.p, b.id.p, sizeof(int32_t) * keep, hipMemcpyDeviceToDevice, c->stream));
        }
        double4 sent = make_double4(MD_SENTINEL_POS, MD_SENTINEL_POS, c->dim == 3 ? MD_SENTINEL_POS : 0.0, 1.0);
        int32_t m1 = -1;
        HIPCHK(hipMemcpyAsync(np.p + newcap, &sent, sizeof(double4), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(ni.p + newcap, &m1, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        std::swap(b.pos.p, np.p);
        std::swap(b.pos.n, np.n);
        std::swap(b.id.p, ni.p);
        std::swap(b.id.n, ni.n);
    }
    c->cap = newcap;
    c->keys_in.ensure(newcap);
    c->keys_out.ensure(newcap);
    c->vals_in.ensure(newcap);
    c->vals_out.ensure(newcap);
    c->gsrc.ensure(newcap + 1);
    c->gcode.ensure(newcap + 1);
    c->gowner.ensure(newcap + 1);
    c->nimg.ensure(newcap + 2);
    c->img_off.ensure(newcap + 2);
    c->newslot.ensure(newcap + 1);
}

void launch_ghost_update(md_ctx *c, int step);

template <int D>
void rebuild_t(md_ctx *c)
{
    hipStream_t st = c->stream;
    c->hess.frozen = false; // (md_hess_*: the slots are about to be renumbered)
    // sources of this build: a single-GPU handle sorts its n particles; a slab handle sorts the
    // survivors of [0, n_old) plus arrivals, plus the x-halo copies received from its neighbours
    const bool dom = c->dom.on;
    const int n_own_src = dom ? (int)(c->dom.n_old + c->dom.n_arr) : (int)c->n;
    const int n_src = dom ? (int)(n_own_src + c->dom.n_xh) : (int)c->n;
    const int32_t *alive = dom ? c->dom.alive.p : nullptr;
    int64_t n_new = dom ? (c->dom.n_old - c->dom.nsend_mig[0] - c->dom.nsend_mig[1] + c->dom.n_arr) : c->n;
    if (n_new > c->ncap) throw HipError("owned-particle capacity exceeded (slab handle: raise n_cap)");
    c->src_count = n_src;
    ensure_capacity(c, n_src + 1);
    int nbs = nblocks(n_src);
    DevState so = c->dev(c->cur);
    BoxGrid g = c->grid;

    // (k_wrap_count also writes the scan's extra item, nimg[n_src] = 0)
    // A slab may own no particle, or have no source at all: a launch with an empty grid is an error, not a no-op.
    if (nbs > 0)
        k_wrap_count<D><<<nbs, MD_BLOCK, 0, st>>>(n_src, n_own_src, so, g, alive, c->nimg.p);
    else
        HIPCHK(hipMemsetAsync(c->nimg.p, 0, sizeof(int32_t), st));
    // exclusive scan over n_src+1 items -> img_off[n_src] = total number of sort entries
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, tmp_bytes, c->nimg.p, c->img_off.p, (int32_t)0, (size_t)n_src + 1,
                                   rocprim::plus<int32_t>(), st));
    c->scan_tmp.ensure(tmp_bytes);
    HIPCHK(rocprim::exclusive_scan(c->scan_tmp.p, tmp_bytes, c->nimg.p, c->img_off.p, (int32_t)0, (size_t)n_src + 1,
                                   rocprim::plus<int32_t>(), st));
    int32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, c->img_off.p + n_src, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t next = total;
    int n = (int)n_new;
    int32_t nghost = (int32_t)(next - n_new);
    if (nghost < 0) throw HipError("internal: fewer sort entries than owned particles");
    ensure_capacity(c, next);
    so = c->dev(c->cur);
    DevState sn = c->dev(c->cur ^ 1);

    // (k_emit also zeroes the cell ranges that k_gather fills in after the sort: nothing reads them in between)
    if (nbs > 0)
        k_emit<D><<<nbs, MD_BLOCK, 0, st>>>(n_src, n_own_src, so, g, alive, c->img_off.p, c->keys_in.p, c->vals_in.p,
                                            c->cell_start.p, c->cell_end.p, c->ncell_ext + 1);
    // Only the (ghost bit, cell) digits are sorted -- three radix passes instead of five.  The sort is stable, so the
    // particles of a cell keep the order they were emitted in (source-slot order), which is as deterministic as the
    // id order the low digits would give.
    unsigned begin_bit = (unsigned)g.id_bits, end_bit = (unsigned)(g.id_bits + g.cell_bits + 1);
    tmp_bytes = 0;
    if (next > 0) {
        HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, c->keys_in.p, c->keys_out.p, c->vals_in.p, c->vals_out.p,
                                         (size_t)next, begin_bit, end_bit, st));
        c->sort_tmp.ensure(tmp_bytes);
        HIPCHK(rocprim::radix_sort_pairs(c->sort_tmp.p, tmp_bytes, c->keys_in.p, c->keys_out.p, c->vals_in.p,
                                         c->vals_out.p, (size_t)next, begin_bit, end_bit, st));
        // (k_gather also resets the build's flags for the first attempt below)
        k_gather<D><<<nblocks(next), MD_BLOCK, 0, st>>>(n, (int)next, so, sn, g, c->keys_out.p, c->vals_out.p,
                                                         c->newslot.p, c->gsrc.p, c->gcode.p, c->cell_start.p,
                                                         c->cell_end.p, c->scal.p);
    }
    if (nghost > 0)
        k_ghost_owner<<<nblocks(nghost), MD_BLOCK, 0, st>>>(nghost, c->gsrc.p, c->newslot.p, c->gowner.p);
    c->cur ^= 1;
    c->next = next;
    c->nghost = nghost;
    c->n = n_new;
    c->nblk = nblocks(n_new);
    c->src_count = n_new;
    int nb = c->nblk;

    // neighbour rows
    double rl2 = c->rl * c->rl;
    c->use_tiles = false;
    c->have_nlist32 = false;
    c->own_first = false;
    bool tile_ok = false;
    const int rs = (c->uniform_sigma && c->pot_kind != POT_POLYDISPERSE && c->pot_kind != POT_LJ_MOD && c->pot_kind != POT_CUSTOM) ? 24 : 32; // LDS record stride of the tiled force kernel
    auto set_tiles = [&](const Scalars &h) {
        size_t bytes = ((size_t)(h.hmax + 1) * rs + 15) & ~(size_t)15;
        if (!(h.halo_overflow) && bytes <= 150 * 1024) {
            c->use_tiles = true;
            c->hstride = h.hmax;
            c->tile_lds = bytes;
            c->tile_rs = rs;
            if (const char *e = getenv("MDHIP_LDS_PAD")) c->tile_lds += (size_t)atoi(e);
            return true;
        }
        return false;
    };
    auto grow_rows = [&]() {
        c->maxn = ((c->maxn * 3 / 2) + 3) & ~3;
        c->nlist.alloc((size_t)c->ntiles * c->maxn * 64);
        c->nlist16.alloc((size_t)c->ntiles * c->maxn * 64);
    };
    if (c->allow_tiles && c->allow_fused_build) {
        // fast path: fused LDS-tiled sweep + halo compaction
        // fp32 sweep radius with a safety margin over fp32 rounding of tile-relative coordinates
        float rl2f = (float)(rl2 * (1.0 + 1.0e-4));
        for (int attempt = 0; attempt < 8; ++attempt) {
            if (attempt > 0 || next == 0) k_reset_flags<<<1, 1, 0, st>>>(c->scal.p);
            if (c->nblk > 0) // (no tile on a slab that owns no particle: the reset flags stand, Hmax = 0)
                k_build_tile<D><<<c->nblk, MD_BT_THREADS, 0, st>>>(n, sn, g, rl2f, c->cell_start.p, c->cell_end.p,
                                                                   c->nlist16.p, c->maxn, c->nneigh.p, c->nmax_tile.p,
                                                                   c->halo.p, c->hcap, c->halo_count.p, c->scal.p,
                                                                   c->dbg_stamps.p, rs, c->allow_own_first ? 1 : 0);
            if (c->dbg_stamps.p && c->nblk > 0) {
                std::vector<long long> hs((size_t)c->nblk * 10);
                HIPCHK(hipMemcpyAsync(hs.data(), c->dbg_stamps.p, hs.size() * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                double acc[9] = {0};
                for (int b = 0; b < c->nblk; ++b)
                    for (int i = 1; i <= 8; ++i) acc[i] += (double)(hs[(size_t)b * 10 + i] - hs[(size_t)b * 10 + i - 1]);
                fprintf(stderr, "[mdhip] build_tile phase cycles/block: cand %.0f sort %.0f uniq %.0f stage %.0f sweep0 %.0f compact %.0f sweep1 %.0f tail %.0f\n",
                        acc[1] / c->nblk, acc[2] / c->nblk, acc[3] / c->nblk, acc[4] / c->nblk, acc[5] / c->nblk,
                        acc[6] / c->nblk, acc[7] / c->nblk, acc[8] / c->nblk);
            }
            Scalars h;
            HIPCHK(hipMemcpyAsync(&h, c->scal.p, sizeof(Scalars), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (getenv("MDHIP_DEBUG"))
                fprintf(stderr, "[mdhip] fused build: Rmax=%d Smax=%d Hmax=%d halo_overflow=%d row_overflow=%d maxn=%d\n",
                        h.dbg_rmax, h.dbg_smax, h.hmax, h.halo_overflow, h.overflow, c->maxn);
            if (h.halo_overflow) break; // some tile does not fit: two-kernel path below
            if (h.overflow) {
                grow_rows();
                continue;
            }
            tile_ok = set_tiles(h);
            c->own_first = tile_ok && c->allow_own_first;
            break;
        }
    }
    if (!tile_ok) {
        for (int attempt = 0; attempt < 8; ++attempt) {
            k_reset_flags<<<1, 1, 0, st>>>(c->scal.p);
            if (nb > 0)
                k_build_list<D><<<nb, MD_BLOCK, 0, st>>>(n, sn, g, rl2, c->cell_start.p, c->cell_end.p, c->nlist.p,
                                                         c->maxn, c->nneigh.p, c->nmax_tile.p, (uint32_t)c->cap,
                                                         c->scal.p);
            Scalars h;
            HIPCHK(hipMemcpyAsync(&h, c->scal.p, sizeof(Scalars), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!h.overflow) break;
            if (attempt == 7) throw HipError("neighbour rows keep overflowing");
            grow_rows();
        }
        c->have_nlist32 = true;
        if (c->allow_tiles) {
            static int attr_dev_mask2 = 0; // per device
            size_t lds = (size_t)MD_HT * 4 + (size_t)MD_HT * 2 + (MD_TILE + 1) * 4;
            if (!(attr_dev_mask2 & (1 << (c->device & 31)))) {
                HIPCHK(hipFuncSetAttribute((const void *)k_tile_localize, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                attr_dev_mask2 |= 1 << (c->device & 31);
            }
            if (c->nblk > 0)
                k_tile_localize<<<c->nblk, MD_TILE, lds, st>>>(c->nlist.p, c->nlist16.p, c->maxn, c->nmax_tile.p,
                                                               (uint32_t)c->cap, c->halo.p, c->hcap, c->halo_count.p,
                                                               c->scal.p, rs);
            Scalars h;
            HIPCHK(hipMemcpyAsync(&h, c->scal.p, sizeof(Scalars), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            set_tiles(h);
        }
    }
    // tiled path: periodic self-image ghosts become (owner, shift) references resolved while staging the halo,
    // and the per-step ghost refresh disappears.  (Under slab decomposition the owner may itself be a received
    // x-halo record: those are real records, refreshed by message, and reference themselves with shift 0.)
    c->virtual_ghosts = c->use_tiles && c->cap < (1ll << 26);
    if (c->virtual_ghosts && nghost > 0 && c->nblk > 0)
        k_halo_virtualize<<<c->nblk, MD_BLOCK, 0, st>>>(n, c->halo.p, c->hcap, c->halo_count.p, c->gowner.p, c->gcode.p);
    if (getenv("MDHIP_ROWSTATS")) {
        std::vector<int32_t> nn((size_t)n), nm((size_t)c->ntiles);
        HIPCHK(hipMemcpyAsync(nn.data(), c->nneigh.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(nm.data(), c->nmax_tile.p, sizeof(int32_t) * c->ntiles, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double mean = 0, padded = 0, sorted_p = 0, p8 = 0, s8 = 0;
        for (int i = 0; i < n; ++i) mean += nn[i];
        for (int w = 0; w < (n + 63) / 64; ++w) { padded += nm[w]; p8 += (nm[w] + 7) & ~7; }
        for (int t0 = 0; t0 + 256 <= n; t0 += 256) {
            std::vector<int> v(nn.begin() + t0, nn.begin() + t0 + 256);
            std::sort(v.begin(), v.end());
            for (int w = 0; w < 4; ++w) { int mx = (v[64 * w + 63] + 3) & ~3; sorted_p += mx; s8 += (mx + 7) & ~7; }
        }
        int nw = (n + 63) / 64;
        fprintf(stderr, "[mdhip] rows: mean %.2f  wave-max(4) %.2f  wave-max(8) %.2f  sorted-within-tile(4) %.2f  (8) %.2f\n",
                mean / n, padded / nw, p8 / nw, sorted_p / nw, s8 / nw);
    }
    c->list_valid = true;
    c->steps_since_build = 0;
    c->st_rebuilds++;
    c->m0 = c->m1 = 1.0; // (md_scale_cell: fresh rows, the full skin again)
    c->scaled0 = c->scaled1 = false;
    deform_reset0(c), deform_reset1(c);
    c->inner_valid = false; // the next force evaluation is a prune step
    // (a slab handle prunes only when its caller schedules prune steps: md_dom_enable_pruning)
    c->prune_on = c->use_tiles && (!c->dom.on || c->dom.prune_enabled) && c->skin > 0.0 && c->inner_skin_req > 0.0 &&
                  c->inner_skin_req < 0.9 * c->skin && c->pot_kind != POT_CUSTOM;
    if (c->prune_on) {
        c->inner_skin = c->inner_skin_req;
        for (int d = 0; d < c->dim; ++d) c->x1[d].ensure(c->ncap);
        c->nlist16_in.ensure((size_t)c->ntiles * c->maxn * 64);
        c->nmax_tile_in.ensure(c->ntiles);
        // inner halo: capacity = what fits the LDS budget that lets one more block reside per CU than the outer image
        // (uniform: 4 x 40 KB; per-particle diameters: 3 x 53 KB), never more than the outer halo itself
        const size_t target = (c->tile_rs == 24) ? (40 * 1024 - 256) : (53 * 1024);
        int cap_in = (int)std::min<size_t>((size_t)c->hstride, target / c->tile_rs - 1);
        if (c->dom.on || getenv("MDHIP_INNER_CAP_OUTER")) cap_in = c->hstride; // (a slab handle's prune step must not fail: see launch_force_tpu)
        c->hcap_in = std::max(cap_in, 1);
        c->tile_lds_in = (((size_t)(c->hcap_in + 1) * c->tile_rs) + 15) & ~(size_t)15;
        c->halo_in.ensure((size_t)c->nblk * c->hcap_in);
        c->halo_in_count.ensure(c->nblk);
    }
}

// md_scale_cell changed the cell under live rows and left the cell grid alone (ghost slots, gowner and the halo lists
// belong to the grid they were built on): the grid of the new cell, and the capacities that follow it as in md_set_skin /
// md_set_cell, just ahead of the build that needs them.  (No row is live here: plain reallocation.)
void regrid_after_scale(md_ctx *c)
{
    configure_grid(c);
    double frac = 1.0;
    for (int d = 0; d < c->dim; ++d) frac *= (double)c->grid.ncx[d] / c->grid.nc[d];
    const int64_t gcap = (int64_t)((frac - 1.0) * 1.3 * c->ncap) + 4096;
    ensure_capacity(c, c->ncap + gcap);
    double dens = (double)c->n_global;
    dens /= c->volume;
    double vol = (c->dim == 3) ? 4.18879020478639 * c->rl * c->rl * c->rl : 3.14159265358979 * c->rl * c->rl;
    int maxn = ((int)(dens * vol * 1.35) + 24 + 3) & ~3;
    if (maxn > c->maxn) {
        c->maxn = maxn;
        c->nlist.alloc((size_t)c->ntiles * c->maxn * 64);
        c->nlist16.alloc((size_t)c->ntiles * c->maxn * 64);
    }
}

void rebuild(md_ctx *c)
{
    if (c->grid_stale) regrid_after_scale(c);
    if (c->dim == 3)
        rebuild_t<3>(c);
    else
        rebuild_t<2>(c);
    HIPCHK(hipGetLastError());
}

void prof_begin(md_ctx *c, int tag = 0)
{
    if (!c->prof) return;
    // (tags 2, 3 -- list builds, prune steps: every one is timed; the stride thins out only the ordinary launches)
    c->prof_open = tag >= 2 || (c->prof_seen[tag]++ % c->prof_stride) == 0;
    if (!c->prof_open) return;
    if (c->prof_used >= c->prof_ev.size()) {
        if (c->prof_ev.size() >= 8192) return;
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        c->prof_ev.emplace_back(a, b);
        c->prof_tag.push_back(0);
    }
    c->prof_tag[c->prof_used] = tag;
    HIPCHK(hipEventRecord(c->prof_ev[c->prof_used].first, c->stream));
}
void prof_end(md_ctx *c)
{
    if (!c->prof || !c->prof_open) return;
    c->prof_open = false;
    if (c->prof_used >= c->prof_ev.size()) return;
    HIPCHK(hipEventRecord(c->prof_ev[c->prof_used].second, c->stream));
    c->prof_used++;
}
void prof_collect(md_ctx *c)
{
    if (c->prof_used == 0) return;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->prof_used; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[i].first, c->prof_ev[i].second));
        if (c->prof_tag[i] == 1) {
            c->prof_kd_ms_acc += ms;
            c->prof_kd_launch_acc++;
        } else if (c->prof_tag[i] == 2) {
            c->prof_rebuild_ms_acc += ms;
            c->prof_rebuild_acc++;
        } else if (c->prof_tag[i] == 3) {
            c->prof_prune_ms_acc += ms;
            c->prof_prune_acc++;
        } else {
            c->prof_ms_acc += ms;
            c->prof_launch_acc++;
        }
    }
    c->prof_used = 0;
}

// rows: 0 = whatever is current (inner rows when valid; a prune step when they are due),
//       1 = outer rows, no pruning (md_compute_forces and friends)
template <int D, int POT, bool UNIFORM>
void launch_force_tpu(md_ctx *c, bool want_uw, bool kick, double dt, int step, int rows)
{
    int n = (int)c->n;
    int nb = c->nblk;
    bool prune_step = rows == 0 && c->prune_on && !c->inner_valid && kick;
    // (inner rows written by a fused prune step index the INNER halo image, which this kernel does not stage: the
    // outer rows serve instead -- a superset, valid as long as the list is)
    // (inner rows whose offsets index the inner halo image need that image staged: every launch through here
    // knows which of the two the current inner rows belong to -- inner_halo_live)
    bool use_inner = rows == 0 && c->inner_valid;
    const uint16_t *rows16 = use_inner ? c->nlist16_in.p : c->nlist16.p;
    const int32_t *rowmax = use_inner ? c->nmax_tile_in.p : c->nmax_tile.p;
    // Inner halo on the classic path.  A slab handle must not fail a prune step from inside the force kernel (its
    // violation flag is all-reduced BEFORE the force kernel of a step): there the inner halo gets the outer halo's
    // capacity -- it can not overflow -- and only the staging traffic shrinks, not the LDS image.
    const bool ih = c->allow_inner_halo && c->prune_on && c->hcap_in > 0 && c->use_tiles;
    const uint32_t *halo_p = c->halo.p;
    int halo_cap = c->hcap;
    const int32_t *halo_cnt = c->halo_count.p;
    size_t lds_bytes = c->tile_lds;
    uint32_t *hin_p = nullptr;
    if (prune_step && ih) {
        hin_p = c->halo_in.p;
        lds_bytes = ((c->tile_lds + 15) & ~(size_t)15) + (c->tile_lds / 8 + 8) * 2; // + the offset translation table
        c->inner_halo_live = true;
    } else if (prune_step) {
        c->inner_halo_live = false;
    } else if (use_inner && c->inner_halo_live) {
        halo_p = c->halo_in.p;
        halo_cap = c->hcap_in;
        halo_cnt = c->halo_in_count.p;
        lds_bytes = c->tile_lds_in;
    }
    DevState s = c->dev(c->cur);
    double rin = c->rc + c->inner_skin;
    if (prune_step) {
        for (int d = 0; d < 3; ++d) s.x1[d] = c->x1[d].p; // the prune step writes the new reference positions
        k_reset_d1<<<1, 1, 0, c->stream>>>(c->scal.p, step);
    }
#define LF(UW, KK)                                                                                                  \
    k_force<D, POT, UNIFORM, UW, KK><<<nb, MD_BLOCK, 0, c->stream>>>(n, s, c->pp, c->nlist.p, c->maxn,              \
                                                                     c->nmax_tile.p, dt, c->partials.p, nb,         \
                                                                     c->scal.p, step)
#define LT(UW, KK, PR)                                                                                              \
    do {                                                                                                            \
        static int attr_dev_mask = 0; /* the attribute is per device: one bit per device id */                      \
        auto kfn = k_force_tile<D, POT, UNIFORM, UW, KK, PR>;                                                       \
        if (!(attr_dev_mask & (1 << (c->device & 31)))) {                                                           \
            HIPCHK(hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,               \
                                       (int)(160 * 1024 - 2048)));                                                  \
            attr_dev_mask |= 1 << (c->device & 31);                                                                 \
        }                                                                                                           \
        kfn<<<nb, MD_TILE, lds_bytes, c->stream>>>(n, s, c->pp, rows16, c->maxn, rowmax, halo_p, halo_cap,          \
                                                   halo_cnt, dt, c->partials.p, nb, c->scal.p, step,                \
                                                   c->nlist16_in.p, c->nmax_tile_in.p, rin * rin,                   \
                                                   c->dbg_stamps.p, hin_p, c->hcap_in, c->halo_in_count.p);         \
    } while (0)
    prof_begin(c, prune_step ? 3 : 0);
    if (c->use_tiles) {
        if (prune_step) {
            if (want_uw)
                LT(true, true, true);
            else
                LT(false, true, true);
        } else if (want_uw) {
            if (kick)
                LT(true, true, false);
            else
                LT(true, false, false);
        } else {
            if (kick)
                LT(false, true, false);
            else
                LT(false, false, false);
        }
    } else if (want_uw) {
        if (kick)
            LF(true, true);
        else
            LF(true, false);
    } else {
        if (kick)
            LF(false, true);
        else
            LF(false, false);
    }
    prof_end(c);
#undef LF
#undef LT
    if (prune_step) {
        c->inner_valid = true;
        c->m1 = 1.0; // (md_scale_cell: fresh inner rows, the full inner skin again)
        deform_reset1(c);
        c->scaled1 = false;
        c->steps_since_prune = 0;
        c->st_prunes++;
    }
}

// user potential: the same two kernels, compiled at run time around the user's evaluate()
void launch_force_custom(md_ctx *c, int dim, bool want_uw, bool kick, double dt, int step)
{
    if (!c->rtc) throw HipError("custom potential selected but no compiled module (md_set_potential_source)");
    int n = (int)c->n;
    DevState s = c->dev(c->cur);
    int nb = c->nblk;
    prof_begin(c);
    if (c->use_tiles && c->tile_lds <= 64 * 1024) {
        // (user potentials always run on the outer rows: no prune-step variant is compiled for them)
        const uint16_t *l16 = c->nlist16.p;
        int maxn = c->maxn;
        const int32_t *nmt = c->nmax_tile.p;
        const uint32_t *halo = c->halo.p;
        int hcap = c->hcap;
        const int32_t *hc = c->halo_count.p;
        double *part = c->partials.p;
        Scalars *sc = c->scal.p;
        uint16_t *rin = nullptr;
        int32_t *nin = nullptr;
        double rin2 = 0.0;
        long long *stamps = nullptr;
        uint32_t *hin = nullptr;
        int hcap_in = 0;
        int32_t *hinc = nullptr;
        void *args[] = {&n, &s, &c->pp, &l16, &maxn, &nmt, &halo, &hcap, &hc, &dt, &part, &nb, &sc, &step, &rin, &nin, &rin2, &stamps,
                        &hin, &hcap_in, &hinc};
        HIPCHK(hipModuleLaunchKernel(c->rtc->tile[dim - 2][want_uw][kick], nb, 1, 1, MD_TILE, 1, 1,
                                     (unsigned)c->tile_lds, c->stream, args, nullptr));
    } else {
        if (!c->have_nlist32) throw HipError("custom potential: halo too large for LDS and no 32-bit rows (set MDHIP_NO_FUSED_BUILD=1)");
        const uint32_t *l32 = c->nlist.p;
        int maxn = c->maxn;
        const int32_t *nmt = c->nmax_tile.p;
        double *part = c->partials.p;
        const Scalars *sc = c->scal.p;
        void *args[] = {&n, &s, &c->pp, &l32, &maxn, &nmt, &dt, &part, &nb, &sc, &step};
        HIPCHK(hipModuleLaunchKernel(c->rtc->global[dim - 2][want_uw][kick], nb, 1, 1, MD_BLOCK, 1, 1, 0, c->stream,
                                     args, nullptr));
    }
    prof_end(c);
}

template <int D>
void launch_force_d(md_ctx *c, bool want_uw, bool kick, double dt, int step, int rows)
{
    bool u = c->uniform_sigma;
    switch (c->pot_kind) {
    case POT_LJ:
        if (u)
            launch_force_tpu<D, POT_LJ, true>(c, want_uw, kick, dt, step, rows);
        else
            launch_force_tpu<D, POT_LJ, false>(c, want_uw, kick, dt, step, rows);
        break;
    case POT_PSEUDOHS:
        if (u)
            launch_force_tpu<D, POT_PSEUDOHS, true>(c, want_uw, kick, dt, step, rows);
        else
            launch_force_tpu<D, POT_PSEUDOHS, false>(c, want_uw, kick, dt, step, rows);
        break;
    case POT_POLYDISPERSE:
        launch_force_tpu<D, POT_POLYDISPERSE, false>(c, want_uw, kick, dt, step, rows);
        break;
    case POT_LJ_MOD:
        launch_force_tpu<D, POT_LJ_MOD, false>(c, want_uw, kick, dt, step, rows);
        break;
    case POT_CUSTOM:
        launch_force_custom(c, D, want_uw, kick, dt, step);
        break;
    default:
        throw HipError("potential kind not available (custom potentials need md_set_potential_source)");
    }
}

void launch_force(md_ctx *c, bool want_uw, bool kick, double dt, int step, int rows = 0)
{
    if (c->dim == 3)
        launch_force_d<3>(c, want_uw, kick, dt, step, rows);
    else
        launch_force_d<2>(c, want_uw, kick, dt, step, rows);
}

void launch_kickdrift(md_ctx *c, bool nvt, double dt, bool check, int step, BussiSrc bs = BussiSrc{})
{
    int n = (int)c->n;
    DevState s = c->dev(c->cur);
    int nb = c->nblk;
    // displacement limits (see k_kickdrift); INFINITY disables the check (rebuild-every-step mode)
    double skin_half = check ? 0.5 * skin_eff(c) : INFINITY;
    double inner_half = check ? (c->inner_valid ? 0.5 * inner_eff(c) : 0.5 * skin_eff(c)) : INFINITY;
    int use_d1 = c->inner_valid ? 1 : 0;
    prof_begin(c, 1);
    if (c->dim == 3) {
        if (nvt)
            k_kickdrift<3, true><<<nb, MD_BLOCK, 0, c->stream>>>(n, s, dt, skin_half, inner_half, use_d1, c->scal.p, step,
                                                                 bs);
        else
            k_kickdrift<3, false><<<nb, MD_BLOCK, 0, c->stream>>>(n, s, dt, skin_half, inner_half, use_d1, c->scal.p, step,
                                                                 bs);
    } else {
        if (nvt)
            k_kickdrift<2, true><<<nb, MD_BLOCK, 0, c->stream>>>(n, s, dt, skin_half, inner_half, use_d1, c->scal.p, step,
                                                                 bs);
        else
            k_kickdrift<2, false><<<nb, MD_BLOCK, 0, c->stream>>>(n, s, dt, skin_half, inner_half, use_d1, c->scal.p, step,
                                                                 bs);
    }
    prof_end(c);
}

void launch_ghost_update(md_ctx *c, int step)
{
    if (c->nghost == 0 || c->virtual_ghosts) return;
    DevState s = c->dev(c->cur);
    int nb = nblocks(c->nghost);
    if (c->dim == 3)
        k_ghost_update<3><<<nb, MD_BLOCK, 0, c->stream>>>((int)c->n, (int)c->nghost, s, c->grid, c->gowner.p,
                                                          c->gcode.p, c->scal.p, step);
    else
        k_ghost_update<2><<<nb, MD_BLOCK, 0, c->stream>>>((int)c->n, (int)c->nghost, s, c->grid, c->gowner.p,
                                                          c->gcode.p, c->scal.p, step);
}

void launch_finalize(md_ctx *c, bool want_uw, bool nvt, double nf, double term1, int step)
{
    k_finalize<<<1, 1024, 0, c->stream>>>(c->nblk, c->partials.p, want_uw ? 1 : 0, nvt ? 1 : 0, nf, term1, c->d_kt.p,
                                          c->d_r1.p, c->d_r2.p, c->scal.p, step);
}

// ---- fused step loop (k_step_tile) ---------------------------------------------------------------------------
bool fused_available(md_ctx *c)
{
    return c->allow_fused && c->use_tiles && c->virtual_ghosts && !c->dom.on && c->pot_kind != POT_CUSTOM && c->skin > 0.0;
}

bool fused_uniform(md_ctx *c)
{
    return c->uniform_sigma && c->pot_kind != POT_POLYDISPERSE && c->pot_kind != POT_LJ_MOD;
}

// plane stride of the state records: owned particles only on a single-GPU handle; a slab handle also keeps the
// records of the x-halo particles (slots behind the owned range) that its neighbours send every step
inline size_t rec_stride(md_ctx *c) { return c->dom.on ? (size_t)c->cap + 1 : (size_t)c->ncap; }

// canonical state arrays -> records of buffer set 0
void fused_enter(md_ctx *c, double dt)
{
    int n = (int)c->n;
    const bool uni = fused_uniform(c);
    const size_t planes = uni ? 3 : 4;
    for (int w = 0; w < 2; ++w) c->rec[w].ensure(rec_stride(c) * planes);
    DevState s = c->dev(c->cur);
    double h2 = (dt * dt) / 2.0;
    c->fz_a = 0;
    if (c->nblk <= 0) return; // (a slab that owns no particle)
    if (c->dim == 3) {
        if (uni)
            k_fuse<3, true><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, c->rec[0].p, rec_stride(c), h2);
        else
            k_fuse<3, false><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, c->rec[0].p, rec_stride(c), h2);
    } else {
        if (uni)
            k_fuse<2, true><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, c->rec[0].p, rec_stride(c), h2);
        else
            k_fuse<2, false><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, c->rec[0].p, rec_stride(c), h2);
    }
    c->fz_a = 0;
}

// latest buffer set -> canonical state arrays (velocities optionally with the pending Bussi rescale applied)
void fused_leave(md_ctx *c, bool apply_scale)
{
    int n = (int)c->n;
    const bool uni = fused_uniform(c);
    if (c->fz_a) {
        // the latest positions / forces live in the other StateBufs' arrays: make them this one's
        StateBufs &a = c->sb[c->cur], &b = c->sb[c->cur ^ 1];
        std::swap(a.pos.p, b.pos.p);
        std::swap(a.pos.n, b.pos.n);
        for (int d = 0; d < c->dim; ++d) {
            std::swap(a.f[d].p, b.f[d].p);
            std::swap(a.f[d].n, b.f[d].n);
        }
    }
    DevState s = c->dev(c->cur);
    const double2 *rec = c->rec[c->fz_a].p;
    int ap = apply_scale ? 1 : 0;
    if (c->nblk <= 0) {
        c->fz_a = 0;
        return;
    }
    if (c->dim == 3) {
        if (uni)
            k_unfuse<3, true><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, rec, rec_stride(c), c->scal.p, ap);
        else
            k_unfuse<3, false><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, rec, rec_stride(c), c->scal.p, ap);
    } else {
        if (uni)
            k_unfuse<2, true><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, rec, rec_stride(c), c->scal.p, ap);
        else
            k_unfuse<2, false><<<c->nblk, MD_BLOCK, 0, c->stream>>>(n, s, rec, rec_stride(c), c->scal.p, ap);
    }
    c->fz_a = 0;
}

template <int D, int POT, bool UNIFORM>
void launch_step_tpu(md_ctx *c, bool want_uw, double dt, int step)
{
    int n = (int)c->n;
    int nb = c->nblk;
    bool prune_step = c->prune_on && !c->inner_valid;
    bool use_inner = c->inner_valid;
    const uint16_t *rows16 = use_inner ? c->nlist16_in.p : c->nlist16.p;
    const int32_t *rowmax = use_inner ? c->nmax_tile_in.p : c->nmax_tile.p;
    // displacement limits of the rows this step walks (k_kickdrift's rule)
    double skin_half = 0.5 * skin_eff(c);
    double inner_half = use_inner ? 0.5 * inner_eff(c) : 0.5 * skin_eff(c);
    int use_d1 = use_inner ? 1 : 0;
    DevState s = c->dev(c->cur); // x1 = the prune positions while the inner rows are valid, else x0
    double rin = c->rc + c->inner_skin;
    const bool whole = c->part.list == nullptr;
    hipStream_t lst = whole ? c->stream : c->part.stream;
    const int grid = whole ? nb : c->part.count;
    if (prune_step) {
        for (int d = 0; d < 3; ++d) s.x1[d] = c->x1[d].p; // the prune step writes the new reference positions
        if (whole) k_reset_d1<<<1, 1, 0, c->stream>>>(c->scal.p, step - 1); // (a split step: the caller did, ahead of all parts)
    }
    // which halo image the launch stages: the outer one (prune steps, and whenever there is no inner halo), or the
    // inner one the last prune step left behind
    // (a fused prune step builds no inner halo -- md_kernels.hpp, k_step_tile; inner rows left behind by a CLASSIC prune
    // step with MDHIP_INNER_HALO=1 index the inner image, which the ordinary fused step then stages)
    const uint32_t *halo_p = c->halo.p;
    int halo_cap = c->hcap;
    const int32_t *halo_cnt = c->halo_count.p;
    size_t lds_bytes = c->tile_lds;
    uint32_t *hin_p = nullptr;
    int own_first = c->own_first ? 1 : 0; // (the outer halo list; an inner halo image keeps its own numbering)
    if (prune_step) {
        c->inner_halo_live = false;
    } else if (use_inner && c->inner_halo_live) {
        halo_p = c->halo_in.p;
        halo_cap = c->hcap_in;
        halo_cnt = c->halo_in_count.p;
        lds_bytes = c->tile_lds_in;
        own_first = 0;
    }
    c->own_first_staged = own_first != 0;
    const int a = c->fz_a;
    StateBufs &A = c->sb[c->cur ^ a], &B = c->sb[c->cur ^ a ^ 1];
    StepBufs sbufs{};
    sbufs.recA = c->rec[a].p;
    sbufs.recB = c->rec[a ^ 1].p;
    sbufs.rstride = rec_stride(c);
    for (int d = 0; d < 3; ++d) {
        sbufs.fA[d] = A.f[d].p;
        sbufs.fB[d] = B.f[d].p;
    }
    sbufs.posB = B.pos.p;
#define LS(UW, PR)                                                                                                  \
    do {                                                                                                            \
        auto kfn = k_step_tile<D, POT, UNIFORM, UW, PR>;                                                            \
        static int attr_dev_mask = 0;                                                                               \
        if (!(attr_dev_mask & (1 << (c->device & 31)))) {                                                           \
            HIPCHK(hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,               \
                                       (int)(160 * 1024 - 2048)));                                                  \
            attr_dev_mask |= 1 << (c->device & 31);                                                                 \
        }                                                                                                           \
        if (grid > 0)                                                                                               \
            kfn<<<grid, MD_TILE, lds_bytes, lst>>>(n, s, sbufs, c->pp, rows16, c->maxn, rowmax, halo_p, halo_cap,   \
                                                   halo_cnt, dt, skin_half, inner_half, use_d1,                     \
                                                   c->partials.p, nb, c->scal.p, step, c->nlist16_in.p,             \
                                                   c->nmax_tile_in.p, rin * rin, c->dbg_stamps.p, hin_p,            \
                                                   c->hcap_in, c->halo_in_count.p, own_first, c->part.list);        \
    } while (0)
    if (whole) prof_begin(c, prune_step ? 3 : 0);
    if (prune_step) {
        if (want_uw)
            LS(true, true);
        else
            LS(false, true);
    } else {
        if (want_uw)
            LS(true, false);
        else
            LS(false, false);
    }
    if (whole) prof_end(c);
#undef LS
    if (!whole && !c->part.last) return; // (more parts of this step follow)
    c->fz_a ^= 1;
    if (prune_step) {
        c->inner_valid = true;
        c->m1 = 1.0; // (md_scale_cell: fresh inner rows, the full inner skin again)
        deform_reset1(c);
        c->scaled1 = false;
        c->steps_since_prune = 0;
        c->st_prunes++;
    }
}

template <int D>
void launch_step_d(md_ctx *c, bool want_uw, double dt, int step)
{
    bool u = c->uniform_sigma;
    switch (c->pot_kind) {
    case POT_LJ:
        if (u)
            launch_step_tpu<D, POT_LJ, true>(c, want_uw, dt, step);
        else
            launch_step_tpu<D, POT_LJ, false>(c, want_uw, dt, step);
        break;
    case POT_PSEUDOHS:
        if (u)
            launch_step_tpu<D, POT_PSEUDOHS, true>(c, want_uw, dt, step);
        else
            launch_step_tpu<D, POT_PSEUDOHS, false>(c, want_uw, dt, step);
        break;
    case POT_POLYDISPERSE:
        launch_step_tpu<D, POT_POLYDISPERSE, false>(c, want_uw, dt, step);
        break;
    case POT_LJ_MOD:
        launch_step_tpu<D, POT_LJ_MOD, false>(c, want_uw, dt, step);
        break;
    default:
        throw HipError("fused step loop: potential kind not available");
    }
}

void launch_step(md_ctx *c, bool want_uw, double dt, int step)
{
    if (c->dim == 3)
        launch_step_d<3>(c, want_uw, dt, step);
    else
        launch_step_d<2>(c, want_uw, dt, step);
}

Scalars read_scalars(md_ctx *c)
{
    Scalars h;
    HIPCHK(hipMemcpyAsync(&h, c->scal.p, sizeof(Scalars), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return h;
}

int fail(md_ctx *c, const char *what)
{
    if (c)
        c->err = what;
    else
        g_create_error = what;
    return 1;
}

} // namespace

// ---- pressure tensor sampler (md_stress.hpp): launches ----------------------------------------------------------
namespace {

template <int D, int POT, bool UNIFORM>
void launch_stress_tpu(md_ctx *c)
{
    int n = (int)c->n;
    int nb = c->nblk;
    DevState s = c->dev(c->cur);
    double *part = c->stress.part.p;
    if (c->use_tiles) {
        static int attr_dev_mask = 0; // the attribute is per device: one bit per device id
        auto kfn = k_stress_tile<D, POT, UNIFORM>;
        if (!(attr_dev_mask & (1 << (c->device & 31)))) {
            HIPCHK(hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(160 * 1024 - 2048)));
            attr_dev_mask |= 1 << (c->device & 31);
        }
        if (c->tile_rs != (UNIFORM ? 24 : 32)) throw HipError("internal: stress sampler and tile rows disagree on the record stride");
        kfn<<<nb, MD_TILE, c->tile_lds, c->stream>>>(n, s, c->pp, c->nlist16.p, c->maxn, c->nmax_tile.p, c->halo.p, c->hcap,
                                                     c->halo_count.p, part, nb);
    } else {
        if (!c->have_nlist32) throw HipError("internal: neither tiled nor 32-bit rows exist");
        k_stress<D, POT, UNIFORM><<<nb, MD_BLOCK, 0, c->stream>>>(n, s, c->pp, c->nlist.p, c->maxn, c->nmax_tile.p, part, nb);
    }
}

template <int D>
void launch_stress_d(md_ctx *c)
{
    bool u = c->uniform_sigma;
    switch (c->pot_kind) {
    case POT_LJ:
        if (u)
            launch_stress_tpu<D, POT_LJ, true>(c);
        else
            launch_stress_tpu<D, POT_LJ, false>(c);
        break;
    case POT_PSEUDOHS:
        if (u)
            launch_stress_tpu<D, POT_PSEUDOHS, true>(c);
        else
            launch_stress_tpu<D, POT_PSEUDOHS, false>(c);
        break;
    case POT_POLYDISPERSE:
        launch_stress_tpu<D, POT_POLYDISPERSE, false>(c);
        break;
    case POT_LJ_MOD:
        launch_stress_tpu<D, POT_LJ_MOD, false>(c);
        break;
    default:
        throw HipError("md_stress_sample: not available with a user potential (MD_POT_CUSTOM)");
    }
}

inline int stress_nc(const md_ctx *c) { return c->dim == 3 ? 6 : 3; }

void stress_zero(md_ctx *c)
{
    md_ctx::Stress &S = c->stress;
    const int nc = stress_nc(c);
    HIPCHK(hipMemsetAsync(S.sums.p, 0, sizeof(double) * 2 * nc, c->stream));
    HIPCHK(hipMemsetAsync(S.ring.p, 0, sizeof(double) * std::max(S.nlags, 1) * nc, c->stream));
    HIPCHK(hipMemsetAsync(S.corr.p, 0, sizeof(double) * std::max(S.nlags, 1) * nc, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    S.nsamples = 0;
}

// ---- the row-walking samplers (md_rowwalk.hpp): one launch decision ---------------------------------------------------
// Tiles or 32-bit rows, the record stride, and -- tiled -- the walk's LDS image.  The rows address the force kernel's image
// with 16-bit byte offsets, (H + 1) * stride <= 65535 for every tile (k_build_tile / k_tile_localize refuse a larger
// halo), so the walk's own 32-byte image always fits below the force kernel's limit (md_rowwalk.hpp asserts the
// arithmetic).  The launch checks the premise on the handle -- the offsets fit 16 bits -- and the conclusion, and refuses
// otherwise.  r2 is the pass's own walk radius; `who` names the sampler in the refusals.
template <int D, class Lane>
void launch_rows(md_ctx *c, double r2, const typename Lane::Args &A, const char *who)
{
    const int n = (int)c->n;
    DevState s = c->dev(c->cur);
    if (!c->use_tiles) {
        if (!c->have_nlist32) throw HipError("internal: neither tiled nor 32-bit rows exist");
        k_rows<D, Lane><<<c->nblk, MD_BLOCK, 0, c->stream>>>(RowsGlobal{n, s, c->nlist.p, c->maxn, c->nmax_tile.p, c->gowner.p},
                                                             r2, A);
        return;
    }
    void (*kern)(RowsTile, double, typename Lane::Args) = c->tile_rs == 24   ? k_rows_tile<D, 24, Lane>
                                                          : c->tile_rs == 32 ? k_rows_tile<D, 32, Lane>
                                                                             : nullptr;
    if (!kern) throw HipError(std::string("internal: ") + who + " sampler and tile rows disagree on the record stride");
    static int attr_dev_mask[2] = {0, 0}; // the attribute is per kernel (stride 24, 32) and per device: one bit per device id
    int &mask = attr_dev_mask[c->tile_rs == 32];
    if (!(mask & (1 << (c->device & 31)))) {
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MD_ROW_LDS_LIMIT));
        mask |= 1 << (c->device & 31);
    }
    if (((size_t)c->hstride + 1) * c->tile_rs > MD_ROW_OFFSET_MAX || !row_image_fits(c->hstride))
        throw HipError(std::string("internal: the ") + who + " sampler's LDS image does not fit");
    kern<<<c->nblk, MD_TILE, row_image_bytes(c->hstride), c->stream>>>(
        RowsTile{n, s, c->nlist16.p, c->maxn, c->nmax_tile.p, c->halo.p, c->hcap, c->halo_count.p, c->gowner.p}, r2, A);
}

// ---- bond-orientational order sampler (md_boo.hpp): launches -----------------------------------------------------
template <int D, int L>
void launch_boo(md_ctx *c)
{
    md_ctx::Boo &B = c->boo;
    int n = (int)c->n;
    int nb = c->nblk;
    B.part.ensure((size_t)BooShape<D, L>::NPART * std::max(nb, 1));
    BooAvgArgs A{};
    A.threshold = B.threshold;
    A.min_conn = B.min_conn;
    A.nbins = B.nbins;
    A.cap = n;
    A.nblk = nb;
    A.bc = B.coef;
    A.qlm = B.qlm.p;
    A.norm = B.norm.p;
    A.nnb = B.nnb.p;
    A.q = B.q.p;
    A.qbar = B.qbar.p;
    A.nconn = B.nconn.p;
    A.hist = B.hist.p;
    A.partials = B.part.p;
    launch_rows<D, BooQlmLane<D, L>>(c, B.rn2, BooQlmArgs{B.order, n, B.coef, B.qlm.p, B.norm.p, B.nnb.p}, "bond-order");
    launch_rows<D, BooAvgLane<D, L>>(c, B.rn2, A, "bond-order");
    k_boo_finish<D, L><<<1, 1024, 0, c->stream>>>(nb, B.part.p, B.coef, (long long)B.nsamples, (long long)B.nseries,
                                                  B.sum_fr.p, B.series.p);
}

// c_lm = (-1)^m sqrt((2l + 1)/(4 pi) (l - m)!/(l + m)!) and 4 pi/(2l + 1); 2-D: 1 and 1
BooCoef boo_coef(int dim, int order)
{
    BooCoef bc{};
    bc.pref = 1.0;
    bc.coef[0] = 1.0;
    if (dim == 2) return bc;
    const double pi = 3.14159265358979323846;
    const int l = order;
    bc.pref = 4.0 * pi / (2 * l + 1);
    for (int m = 0; m <= l; ++m) {
        double ratio = 1.0; // (l - m)! / (l + m)!
        for (int k = l - m + 1; k <= l + m; ++k) ratio /= (double)k;
        bc.coef[m] = ((m & 1) ? -1.0 : 1.0) * std::sqrt((2 * l + 1) / (4.0 * pi) * ratio);
    }
    return bc;
}

void boo_zero(md_ctx *c)
{
    md_ctx::Boo &B = c->boo;
    HIPCHK(hipMemsetAsync(B.sum_fr.p, 0, sizeof(double) * MD_BOO_NFR, c->stream));
    HIPCHK(hipMemsetAsync(B.series.p, 0, sizeof(double) * MD_BOO_NFR * std::max<int64_t>(B.nseries, 1), c->stream));
    HIPCHK(hipMemsetAsync(B.hist.p, 0, sizeof(unsigned long long) * B.nhist(), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    B.nsamples = 0;
}

// ---- marked pair correlations (md_mpc.hpp): launches ----------------------------------------------------------------
template <int D, int NC>
void mpc_set_lds(size_t lds)
{
    HIPCHK(hipFuncSetAttribute((const void *)k_mpc_hist<D, NC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
}

template <int D, int NC>
void mpc_launch(md_ctx *ctx, const double *src, const int32_t *inv, size_t stride_i, size_t stride_c, size_t lds)
{
    md_ctx::Mpc &M = ctx->mpc;
    const int n = (int)ctx->n;
    const RdfGrid &g = M.grid;
    hipStream_t st = ctx->stream;
    k_mpc_gather<NC><<<nblocks(n), MD_BLOCK, 0, st>>>(n, M.keys_out.p, M.vals_out.p, M.wrec.p, src, inv, stride_i, stride_c,
                                                      M.w, M.srec.p, M.smarks.p, M.cell_start.p, M.cell_end.p, M.self.p,
                                                      M.range_error.p);
    HIPCHK(hipGetLastError());
    // one wave per home cell at a time, cells handed out by the work counter; the grid only needs to fill the chip
    const int waves_per_block = MD_RDF_BLOCK / 64;
    const int nblk = (int)std::min<int64_t>((g.ncell + waves_per_block - 1) / waves_per_block, 1024);
    const float inv_delta = (float)(M.nbins / M.r_max);
    k_mpc_hist<D, NC><<<nblk, MD_RDF_BLOCK, lds, st>>>(g, M.nbins, inv_delta, M.w, M.e2.p, M.srec.p, M.smarks.p,
                                                       M.cell_start.p, M.cell_end.p, M.work.p, M.cur_cnt.p,
                                                       (unsigned long long *)M.cur_sum.p, M.range_error.p);
    HIPCHK(hipGetLastError());
}

// the instantiations: D = 2 with NC in {1, 2, 3}; D = 3 with NC in {1, 2, 3, 10, 14}
template <class F2, class F3>
void mpc_dispatch(int dim, int nc, F2 &&two, F3 &&three)
{
    if (dim == 2) {
        switch (nc) {
        case 1: two(std::integral_constant<int, 1>{}); return;
        case 2: two(std::integral_constant<int, 2>{}); return;
        case 3: two(std::integral_constant<int, 3>{}); return;
        }
    } else {
        switch (nc) {
        case 1: three(std::integral_constant<int, 1>{}); return;
        case 2: three(std::integral_constant<int, 2>{}); return;
        case 3: three(std::integral_constant<int, 3>{}); return;
        case 10: three(std::integral_constant<int, 10>{}); return;
        case 14: three(std::integral_constant<int, 14>{}); return;
        }
    }
    throw HipError("md_mpc: no kernel for this dimension and number of mark components");
}

size_t mpc_lds_bytes(int nbins, int nc)
{
    return sizeof(double) * (size_t)(MD_RDF_BLOCK * nc + MD_MPC_MAX_NC + 2) + sizeof(double) * (nbins + 1) + sizeof(uint32_t) * nbins +
           sizeof(long long) * nbins;
}

void mpc_zero(md_ctx *c)
{
    md_ctx::Mpc &M = c->mpc;
    hipStream_t st = c->stream;
    const size_t nb = (size_t)M.nbins;
    HIPCHK(hipMemsetAsync(M.cur_cnt.p, 0, sizeof(unsigned long long) * nb, st));
    HIPCHK(hipMemsetAsync(M.cur_sum.p, 0, sizeof(long long) * nb, st));
    HIPCHK(hipMemsetAsync(M.last_cnt.p, 0, sizeof(unsigned long long) * nb, st));
    HIPCHK(hipMemsetAsync(M.last_sum.p, 0, sizeof(long long) * nb, st));
    HIPCHK(hipMemsetAsync(M.acc_cnt.p, 0, sizeof(unsigned long long) * nb, st));
    HIPCHK(hipMemsetAsync(M.acc_sum.p, 0, sizeof(double) * nb, st));
    HIPCHK(hipMemsetAsync(M.self.p, 0, sizeof(long long) * 2, st));
    HIPCHK(hipMemsetAsync(M.acc_self.p, 0, sizeof(double), st));
    HIPCHK(hipMemsetAsync(M.range_error.p, 0, sizeof(int32_t), st));
    HIPCHK(hipStreamSynchronize(st));
    M.nsamples = 0;
    M.sampled = false;
}

// ---- cluster sampler (md_cluster.hpp): launches -------------------------------------------------------------------
template <int D>
void launch_cluster(md_ctx *c)
{
    md_ctx::Cluster &C = c->cluster;
    md_ctx::Boo &B = c->boo;
    const int n = (int)c->n, nb = nblocks(c->n), nh = c->nblk;
    hipStream_t st = c->stream;
    DevState s = c->dev(c->cur);
    C.deg.ensure((size_t)std::max(nh, 1));
    const bool solid = C.members == MD_CLUSTER_SOLID;
    if (solid) k_cl_mask<<<nb, MD_BLOCK, 0, st>>>(n, B.ids.p, B.nconn.p, B.min_conn, C.mask.p);
    k_cl_init<<<nb, MD_BLOCK, 0, st>>>(n, s.id, solid ? C.mask.p : nullptr, C.parent.p, C.mem.p, C.count.p, C.minid.p);
    launch_rows<D, ClLane>(c, C.rb2, ClArgs{C.mem.p, C.parent.p, C.deg.p}, "cluster");
    k_cl_flatten<<<nb, MD_BLOCK, 0, st>>>(n, s.id, C.parent.p, C.root.p, C.count.p, C.minid.p);
    k_cl_stats<<<nb, MD_BLOCK, 0, st>>>(n, C.root.p, C.count.p, C.minid.p, C.max_size, C.hist.p, nb, C.part.p);
    k_cl_finish<<<1, 1024, 0, st>>>(nb, C.part.p, nh, C.deg.p, (long long)C.nsamples, (long long)C.nseries, C.sum_fr.p,
                                    C.series.p);
}

void cluster_zero(md_ctx *c)
{
    md_ctx::Cluster &C = c->cluster;
    HIPCHK(hipMemsetAsync(C.sum_fr.p, 0, sizeof(long long) * MD_CL_NFR, c->stream));
    HIPCHK(hipMemsetAsync(C.series.p, 0, sizeof(long long) * MD_CL_NFR * std::max<int64_t>(C.nseries, 1), c->stream));
    HIPCHK(hipMemsetAsync(C.hist.p, 0, sizeof(unsigned long long) * ((size_t)C.max_size + 1), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    C.nsamples = 0;
}

// ---- the time-correlation samplers (md_dyn.hpp, md_sq.hpp, md_cage.hpp, md_chi4.hpp) ---------------------------------
// What setup and reset share: the accumulators and the row counts set to zero, and a wait.
void dyn_zero(md_ctx *c)
{
    md_ctx::Dyn &Y = c->dyn;
    HIPCHK(hipMemsetAsync(Y.sums.p, 0, sizeof(double) * Y.sr.nrows * (2 + Y.nq), c->stream));
    HIPCHK(hipMemsetAsync(Y.hist.p, 0, sizeof(unsigned long long) * Y.sr.nrows * std::max(Y.nbins, 1), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    Y.sr.clear_counts();
}

void sq_zero(md_ctx *c)
{
    md_ctx::Sq &S = c->sq;
    HIPCHK(hipMemsetAsync(S.s2.p, 0, sizeof(double) * S.nvec, c->stream));
    if (S.sr.nrows) HIPCHK(hipMemsetAsync(S.corr.p, 0, sizeof(double) * S.sr.nrows * S.nvec, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    S.nstatic = 0;
    S.sr.clear_counts();
}

// The DynParams of a sample against the current cell: n, dim, U and nblk; with q, the nq wave numbers and nquant = 2 + nq
// (0 without: md_chi4's kernels read n and U alone); with nbins > 0, the van Hove bins.
DynParams dyn_params(const md_ctx *c, const std::vector<double> *q = nullptr, int nbins = 0, double r_max = 0.0)
{
    DynParams P{};
    P.n = (int)c->n;
    P.dim = c->dim;
    P.nblk = blocks_of(c->n, MD_DYN_BLOCK * MD_DYN_PPT);
    for (int k = 0; k < 9; ++k) P.U[k] = c->A[k];
    if (q) {
        P.nq = (int)q->size();
        P.nquant = 2 + P.nq;
        std::copy(q->begin(), q->end(), P.q);
    }
    P.nbins = nbins;
    P.inv_delta = nbins > 0 ? (float)(nbins / r_max) : 0.0f;
    return P;
}

// Entries i0.. of a sample call's (slot, row) pairs, as many as one launch takes
template <class Batch>
Batch batch_from(const int32_t *slots, const int32_t *rows, int i0, int count, int max_batch)
{
    Batch B{};
    B.count = std::min(count - i0, max_batch);
    std::copy(slots + i0, slots + i0 + B.count, B.slot);
    std::copy(rows + i0, rows + i0 + B.count, B.row);
    return B;
}

// A sample call's (slot, row) pairs batch by batch: fn(B, first, last) -- once with an empty batch when count == 0, for
// the samplers whose launch also reduces the frame and stores the origin (md_sq, md_cur)
template <class Batch, class F>
void for_batches(const int32_t *slots, const int32_t *rows, int count, int max_batch, F fn)
{
    int i0 = 0;
    do {
        const Batch B = batch_from<Batch>(slots, rows, i0, count, max_batch);
        const bool first = i0 == 0;
        i0 += B.count;
        fn(B, first, i0 >= count);
    } while (i0 < count);
}

// ---- cage-relative dynamics (md_cage.hpp): launches ----------------------------------------------------------------
// The origin walk's own test is the list cutoff (the rows are complete up to it); the bond criterion is the lane's.
template <int D>
void launch_cage_origin(md_ctx *c, int slot)
{
    md_ctx::Cage &G = c->cage;
    const size_t n = (size_t)c->n, mn = (size_t)G.max_neigh;
    CageOrigin T{};
    T.n = (int)n;
    T.max_neigh = G.max_neigh;
    T.scaled = G.scaled;
    T.r_neigh = G.r_neigh;
    T.nnb = G.nnb.p + (size_t)slot * n;
    T.nid = G.nid.p + (size_t)slot * mn * n;
    T.del = G.del.p + (size_t)slot * mn * D * n;
    T.sig = G.sig.p + (size_t)slot * n;
    T.overflow = G.overflow.p;
    launch_rows<D, CageOriginLane<D>>(c, c->rc * c->rc, T, "cage");
}

template <int D>
void launch_cage_sample(md_ctx *c, const DynParams &P, const DynBatch &B, const CageSample &A)
{
    md_ctx::Cage &G = c->cage;
    hipStream_t st = c->stream;
    dim3 g1((unsigned)((c->n + MD_DYN_BLOCK - 1) / MD_DYN_BLOCK), B.count), g2(P.nblk, B.count);
    k_cage_disp<D><<<g1, MD_DYN_BLOCK, 0, st>>>(P, B, G.cx.p, G.ci.p, G.ox.p, G.oi.p, G.disp.p);
    k_cage_sample<D><<<g2, MD_DYN_BLOCK, 0, st>>>(P, B, A);
    k_dyn_reduce<<<1, MD_DYN_REDUCE_BLOCK, 0, st>>>(P, B, G.part.p, G.sums.p);
}

void cage_zero(md_ctx *c)
{
    md_ctx::Cage &G = c->cage;
    const size_t nr = (size_t)G.sr.nrows;
    HIPCHK(hipMemsetAsync(G.sums.p, 0, sizeof(double) * nr * (2 + G.nq), c->stream));
    HIPCHK(hipMemsetAsync(G.counts.p, 0, sizeof(unsigned long long) * nr * MD_CAGE_NCOUNT, c->stream));
    HIPCHK(hipMemsetAsync(G.hist.p, 0, sizeof(unsigned long long) * nr * MD_CAGE_NHIST, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    G.sr.clear_counts();
}

// ---- four-point dynamics (md_chi4.hpp): launches ---------------------------------------------------------------------

// One (slot, row) sample against the current frame in cx / ci: three launches (two when there are no vectors).
template <int D>
void launch_chi4_sample(md_ctx *c, const DynParams &P, int slot, int row)
{
    md_ctx::Chi4 &X = c->chi4;
    hipStream_t st = c->stream;
    const size_t frame = (size_t)P.n * D;
    const int oblk = (P.n + MD_CHI4_BLOCK * MD_CHI4_PPT - 1) / (MD_CHI4_BLOCK * MD_CHI4_PPT);
    k_chi4_overlap<D><<<oblk, MD_CHI4_BLOCK, 0, st>>>(P, X.a2, X.cx.p, X.ci.p, X.ox.p + (size_t)slot * frame,
                                                      X.oi.p + (size_t)slot * frame, X.mask.p, X.qcur.p);
    if (X.nvec > 0)
        k_chi4_modes<D><<<dim3(X.nblk, X.nvec_pad / MD_SQ_TILE), MD_SQ_BLOCK, 0, st>>>(
            P.n, X.nblk, X.of.p + (size_t)slot * frame, X.nd.p, X.part.p, X.mask.p, X.nwords);
    const int rblk = std::max(1, (X.nvec + MD_SQ_REDUCE_BLOCK / 64 - 1) / (MD_SQ_REDUCE_BLOCK / 64));
    k_chi4_reduce<<<rblk, MD_SQ_REDUCE_BLOCK, 0, st>>>(X.nvec, X.nblk, X.part.p, X.wlast.p,
                                                       X.s4.p + (size_t)row * std::max(X.nvec, 1), X.qcur.p, X.qlast.p,
                                                       X.irow.p + (size_t)row * MD_CHI4_NROW);
    HIPCHK(hipGetLastError());
}

void chi4_zero(md_ctx *c)
{
    md_ctx::Chi4 &X = c->chi4;
    HIPCHK(hipMemsetAsync(X.irow.p, 0, sizeof(long long) * X.sr.nrows * MD_CHI4_NROW, c->stream));
    HIPCHK(hipMemsetAsync(X.s4.p, 0, sizeof(double) * X.sr.nrows * std::max(X.nvec, 1), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    X.sr.clear_counts();
}

// ---- currents (md_cur.hpp): launches ---------------------------------------------------------------------------------
template <int D>
void launch_cur_modes(md_ctx *c, hipStream_t st)
{
    md_ctx::Cur &S = c->current;
    const int n = (int)c->n;
    k_cur_vaxis<D><<<nblocks(n), MD_BLOCK, 0, st>>>(n, S.cv.p, S.va.p);
    const int ntiles = S.nvec_pad / MD_CUR_TILE;
    k_cur_modes<D><<<(unsigned)S.nblk * (unsigned)ntiles, MD_CUR_BLOCK, 0, st>>>(n, S.nblk, ntiles, S.fr.p, S.va.p, S.nd.p,
                                                                              S.part.p);
    HIPCHK(hipGetLastError());
}

template <int D>
void launch_cur_reduce(md_ctx *c, hipStream_t st, bool first, bool add_static, const CurBatch &B, int origin_slot)
{
    md_ctx::Cur &S = c->current;
    const int rblk = (S.nvec + MD_CUR_REDUCE_BLOCK / 64 - 1) / (MD_CUR_REDUCE_BLOCK / 64);
    k_cur_reduce<D><<<rblk, MD_CUR_REDUCE_BLOCK, 0, st>>>(S.nvec, S.nblk, first, add_static, B, origin_slot, S.part.p,
                                                        S.e.p, S.jl.p, S.s_tot.p, S.s_long.p, S.c_tot.p, S.c_long.p,
                                                        S.org.p);
    HIPCHK(hipGetLastError());
}

void cur_zero(md_ctx *c)
{
    md_ctx::Cur &S = c->current;
    const size_t nr = (size_t)S.sr.nrows;
    if (S.nvec) {
        HIPCHK(hipMemsetAsync(S.s_tot.p, 0, sizeof(double) * S.nvec, c->stream));
        HIPCHK(hipMemsetAsync(S.s_long.p, 0, sizeof(double) * S.nvec, c->stream));
        if (nr) HIPCHK(hipMemsetAsync(S.c_tot.p, 0, sizeof(double) * nr * S.nvec, c->stream));
        if (nr) HIPCHK(hipMemsetAsync(S.c_long.p, 0, sizeof(double) * nr * S.nvec, c->stream));
    }
    if (S.vacf) HIPCHK(hipMemsetAsync(S.z.p, 0, sizeof(double) * (nr + 1), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    S.nstatic = 0;
    S.sr.clear_counts();
}

// ---- swap Monte Carlo (md_swap.hpp): the walk's launch ------------------------------------------------------------
template <int D>
void launch_swap_walk(md_ctx *c, const SwapRows &V, const DevState &s, const SwapBufs &B, int grid)
{
    const double c2 = c->rc * c->rc;
    switch (c->pot_kind) {
    case POT_LJ:
        k_swap_walk<D, POT_LJ><<<grid, MD_BLOCK, 0, c->stream>>>(V, s, c->pp, c2, B);
        break;
    case POT_PSEUDOHS:
        k_swap_walk<D, POT_PSEUDOHS><<<grid, MD_BLOCK, 0, c->stream>>>(V, s, c->pp, c2, B);
        break;
    case POT_POLYDISPERSE:
        k_swap_walk<D, POT_POLYDISPERSE><<<grid, MD_BLOCK, 0, c->stream>>>(V, s, c->pp, c2, B);
        break;
    case POT_LJ_MOD:
        k_swap_walk<D, POT_LJ_MOD><<<grid, MD_BLOCK, 0, c->stream>>>(V, s, c->pp, c2, B);
        break;
    default:
        throw HipError("md_swap_rounds: potential kind not available");
    }
}

// ---- Hessian of the pair energy (md_hess.hpp): launches ---------------------------------------------------------------
// One apply kernel, two host entry paths: md_hess_apply stages host blocks into slot order around it, the Lanczos loop and
// md_hess_ritz hand it resident vectors.  X and Y are [slot][M][D]; M is 1, 4 or 8 (hess_block pads a block with zero vectors).
inline int hess_block(int m) { return m <= 1 ? 1 : (m <= 4 ? 4 : MD_HESS_MAX_M); }

HessPairArgs hess_pair_args(md_ctx *c)
{
    HessPairArgs P{};
    P.pp = c->pp;
    for (int i = 0; i < 9; ++i) P.Ainv[i] = c->Ainv[i];
    return P;
}

template <int D, int POT>
void launch_hess_apply_p(md_ctx *c, int M, const double *X, double *Y)
{
    HessApplyArgs A{hess_pair_args(c), X, Y};
    switch (M) {
    case 1:
        launch_rows<D, HessApplyLane<D, POT, 1>>(c, c->pp.c2, A, "Hessian");
        break;
    case 4:
        launch_rows<D, HessApplyLane<D, POT, 4>>(c, c->pp.c2, A, "Hessian");
        break;
    case MD_HESS_MAX_M:
        launch_rows<D, HessApplyLane<D, POT, MD_HESS_MAX_M>>(c, c->pp.c2, A, "Hessian");
        break;
    default:
        throw HipError("internal: no Hessian apply kernel for this block size");
    }
}

template <int D, int POT>
void launch_hess_diag_p(md_ctx *c, int, const double *, double *diag)
{
    launch_rows<D, HessDiagLane<D, POT>>(c, c->pp.c2, HessDiagArgs{hess_pair_args(c), diag}, "Hessian");
}

#define MD_HESS_DISPATCH(fn, c, M, X, Y)                                                                            \
    do {                                                                                                            \
        const bool d3_ = (c)->dim == 3;                                                                             \
        switch ((c)->pot_kind) {                                                                                    \
        case POT_LJ:                                                                                                \
            d3_ ? fn<3, POT_LJ>(c, M, X, Y) : fn<2, POT_LJ>(c, M, X, Y);                                            \
            break;                                                                                                  \
        case POT_PSEUDOHS:                                                                                          \
            d3_ ? fn<3, POT_PSEUDOHS>(c, M, X, Y) : fn<2, POT_PSEUDOHS>(c, M, X, Y);                                \
            break;                                                                                                  \
        case POT_POLYDISPERSE:                                                                                      \
            d3_ ? fn<3, POT_POLYDISPERSE>(c, M, X, Y) : fn<2, POT_POLYDISPERSE>(c, M, X, Y);                        \
            break;                                                                                                  \
        case POT_LJ_MOD:                                                                                            \
            d3_ ? fn<3, POT_LJ_MOD>(c, M, X, Y) : fn<2, POT_LJ_MOD>(c, M, X, Y);                                    \
            break;                                                                                                  \
        default:                                                                                                    \
            throw HipError("md_hess: not available with a user potential (MD_POT_CUSTOM)");                         \
        }                                                                                                           \
        HIPCHK(hipGetLastError());                                                                                  \
    } while (0)

void launch_hess_apply(md_ctx *c, int M, const double *X, double *Y) { MD_HESS_DISPATCH(launch_hess_apply_p, c, M, X, Y); }
void launch_hess_diag(md_ctx *c, double *diag) { MD_HESS_DISPATCH(launch_hess_diag_p, c, 0, (const double *)nullptr, diag); }

// The operator of the frame the handle holds, or a refusal: never a stale frame.
md_ctx::Hess &hess_of(md_ctx *ctx, const char *who)
{
    if (ctx->dom.on) throw HipError(std::string(who) + ": not available on a slab-decomposition handle");
    if (ctx->pot_kind == POT_CUSTOM) throw HipError(std::string(who) + ": not available with a user potential (MD_POT_CUSTOM)");
    if (!ctx->hess.frozen || !ctx->list_valid || ctx->state_invalid)
        throw HipError(std::string(who) + ": no operator for the frame the handle holds now (md_upload, md_run*, md_fire_minimize, "
                                          "md_swap_rounds, a change of the potential or a list rebuild since md_hess_setup "
                                          "invalidate it): call md_hess_setup");
    return ctx->hess;
}

// ---- elastic moduli (md_elas.hpp): launches ---------------------------------------------------------------------------
template <int D, int POT>
void launch_elas_affine_p(md_ctx *c, int, const double *, double *)
{
    md_ctx::Elas &E = c->elas;
    ElasAffineArgs A{hess_pair_args(c), E.xi.p, E.bonded.p, E.part.p, c->nblk};
    launch_rows<D, ElasAffineLane<D, POT>>(c, c->pp.c2, A, "elasticity");
}

void launch_elas_affine(md_ctx *c) { MD_HESS_DISPATCH(launch_elas_affine_p, c, 0, (const double *)nullptr, (double *)nullptr); }

// The operator md_hess_setup froze, with the affine pass of that very operator when `need_affine`
md_ctx::Elas &elas_of(md_ctx *ctx, const char *who, bool need_affine)
{
    md_ctx::Hess &H = hess_of(ctx, who);
    if (need_affine && ctx->elas.epoch != H.epoch)
        throw HipError(std::string(who) + ": no affine pass for the operator the last md_hess_setup froze (call md_elas_affine first)");
    return ctx->elas;
}

// The solver's launches for one dimension: M = hess_block(nc) vectors, npair = n M (slot, vector) pairs in nchunk chunks
template <int D>
struct ElasLaunch {
    static constexpr int M = ElasShape<D>::M;
    md_ctx *c;
    ElasVecs V;
    int nchunk;
    double tol;
    hipStream_t st;
    void scalars(int mode) { k_elas_scalars<<<1, MD_BLOCK, 0, st>>>(nchunk, M, mode, tol, V.partials, V.sc); }
    void mean_of(const double *src, const double *nbonded, double *mean)
    {
        k_elas_colsum<D, M><<<nchunk, MD_BLOCK, 0, st>>>(V.npair, src, V.partials);
        k_elas_mean_finish<<<M * D, MD_BLOCK, 0, st>>>(nchunk, V.partials, nbonded, mean);
    }
    void init() { k_elas_init<D, M><<<nchunk, MD_BLOCK, 0, st>>>(V); scalars(0); }
    void iterate()
    {
        launch_hess_apply(c, M, V.p, V.hp);
        k_elas_php<D, M><<<nchunk, MD_BLOCK, 0, st>>>(V);
        scalars(1);
        k_elas_update<D, M><<<nchunk, MD_BLOCK, 0, st>>>(V);
        scalars(2);
        k_elas_direction<D, M><<<nchunk, MD_BLOCK, 0, st>>>(V);
    }
    void project() { k_elas_project<D, M><<<nchunk, MD_BLOCK, 0, st>>>(V); }
    void residual(double *out)
    {
        launch_hess_apply(c, M, V.x, V.hp);
        k_elas_resid<D, M><<<nchunk, MD_BLOCK, 0, st>>>(V);
        k_elas_sum_finish<<<M, MD_BLOCK, 0, st>>>(nchunk, V.partials, 1.0, 1, out);
    }
    void contract(double inv_v, double *part, double *out)
    {
        constexpr int NC = ElasShape<D>::NC;
        k_elas_contract<D><<<c->nblk, MD_BLOCK, 0, st>>>((int)c->n, V.xi, V.x, part);
        k_elas_sum_finish<<<NC * NC, MD_BLOCK, 0, st>>>(c->nblk, part, inv_v, 0, out);
    }
};

template <int D>
void elas_solve_t(md_ctx *ctx, double tol, int64_t max_iter, int64_t *iters, double *resid, double *xi_norm, int *status,
                  double *nonaffine, double *u)
{
    constexpr int NC = ElasShape<D>::NC, NB = ElasShape<D>::NB, M = ElasShape<D>::M;
    md_ctx::Elas &E = ctx->elas;
    const int n = (int)ctx->n;
    const size_t ne = (size_t)n * M * D, npair = (size_t)n * M;
    const int nchunk = (int)((npair + MD_ELAS_CHUNK - 1) / MD_ELAS_CHUNK);
    hipStream_t st = ctx->stream;
    E.x.ensure(ne);
    E.r.ensure(ne);
    E.p.ensure(ne);
    E.hp.ensure(ne);
    E.part.ensure(std::max((size_t)M * D * nchunk, std::max((size_t)NC * NC, (size_t)ElasShape<D>::NQ) * ctx->nblk));
    E.mean.ensure(M * D);
    E.out.ensure(M + NC * NC);
    E.sc.ensure(1);
    ElasLaunch<D> L{ctx, ElasVecs{npair, E.bonded.p, E.xi.p, E.x.p, E.r.p, E.p.p, E.hp.p, E.part.p, E.sc.p, E.mean.p}, nchunk, tol, st};
    const double *nbonded = E.sums.p + NC + NB;
    // the right-hand side, once against the translations of the bonded particles
    L.mean_of(E.xi.p, nbonded, E.mean.p);
    L.init();
    HIPCHK(hipGetLastError());
    ElasScal hs{};
    auto poll = [&]() {
        HIPCHK(hipMemcpyAsync(&hs, E.sc.p, sizeof hs, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    };
    poll();
    int64_t it = 0;
    while (it < max_iter && hs.nactive > 0) { // the host waits once per 32 iterations (md_fire_minimize's convention)
        const int64_t chunk_end = std::min<int64_t>(max_iter, it + 32);
        for (; it < chunk_end; ++it) L.iterate();
        HIPCHK(hipGetLastError());
        poll();
    }
    // the solution, once against the same translations; then the true residual and the contraction
    L.mean_of(E.x.p, nbonded, E.mean.p);
    L.project();
    L.residual(E.out.p);
    L.contract(1.0 / ctx->volume, E.part.p, E.out.p + M);
    HIPCHK(hipGetLastError());
    double ho[MD_HESS_MAX_M + 36];
    HIPCHK(hipMemcpyAsync(ho, E.out.p, sizeof(double) * (M + NC * NC), hipMemcpyDeviceToHost, st));
    if (u) {
        E.host_io.ensure((size_t)n * NC * D);
        k_hess_export<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, ctx->dev(ctx->cur).id, D, NC, M, E.x.p, E.host_io.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(u, E.host_io.p, sizeof(double) * (size_t)n * NC * D, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    int bits = 0;
    bool all_conv = true;
    for (int v = 0; v < NC; ++v) {
        iters[v] = (int64_t)hs.iters[v];
        resid[v] = ho[v];
        xi_norm[v] = std::sqrt(hs.rr0[v]);
        if (hs.state[v] == MD_ELAS_ST_INDEFINITE) bits |= MD_ELAS_INDEFINITE;
        if (hs.state[v] == MD_ELAS_ST_ACTIVE) bits |= MD_ELAS_MAX_ITER;
        if (hs.state[v] != MD_ELAS_ST_CONVERGED) all_conv = false;
    }
    if (all_conv) bits |= MD_ELAS_CONVERGED;
    *status = bits;
    for (int q = 0; q < NC * NC; ++q) nonaffine[q] = ho[M + q];
}

// One Gram-Schmidt pass of w against the translations and the first nb basis vectors; mode / qa / out: k_hess_dots_finish
void hess_gs_pass(md_ctx *c, int nb, int mode, double *out)
{
    md_ctx::Hess &H = c->hess;
    const int D = c->dim;
    const size_t nd = (size_t)c->n * D;
    const int nchunk = (int)((nd + MD_HESS_CHUNK - 1) / MD_HESS_CHUNK);
    const int nq = D + nb;
    const double rsn = 1.0 / std::sqrt((double)c->n);
    hipStream_t st = c->stream;
    k_hess_dots<<<dim3(nchunk, (nq + MD_HESS_QPB - 1) / MD_HESS_QPB), MD_BLOCK, 0, st>>>(nd, D, rsn, H.basis.p, H.w.p, 0, nq, 0, H.part.p);
    k_hess_dots_finish<<<nq, MD_BLOCK, 0, st>>>(nchunk, H.part.p, H.coef.p, mode, nq - 1, out);
    k_hess_update<<<(unsigned)((nd + MD_BLOCK - 1) / MD_BLOCK), MD_BLOCK, 0, st>>>(nd, D, rsn, H.basis.p, H.coef.p, nq, H.w.p);
}

// |w| into norm_out[0], then (dst != nullptr) dst = w / |w|
void hess_normalise(md_ctx *c, double *norm_out, double *dst)
{
    md_ctx::Hess &H = c->hess;
    const size_t nd = (size_t)c->n * c->dim;
    const int nchunk = (int)((nd + MD_HESS_CHUNK - 1) / MD_HESS_CHUNK);
    hipStream_t st = c->stream;
    k_hess_dots<<<nchunk, MD_BLOCK, 0, st>>>(nd, c->dim, 0.0, H.basis.p, H.w.p, 0, 1, 1, H.part.p);
    k_hess_dots_finish<<<1, MD_BLOCK, 0, st>>>(nchunk, H.part.p, H.coef.p, 3, -1, norm_out);
    if (dst) k_hess_scale<<<(unsigned)((nd + MD_BLOCK - 1) / MD_BLOCK), MD_BLOCK, 0, st>>>(nd, H.w.p, norm_out, dst);
}

} // namespace

struct FusedScope { // md_run / slab windows: marks the handle's state invalid when the fused loop is left by an exception
    md_ctx *c;
    bool done = false;
    ~FusedScope()
    {
        if (!done) c->state_invalid = true;
    }
};

inline void require_state(md_ctx *c, const char *who)
{
    if (c->state_invalid)
        throw HipError(std::string(who) + ": an earlier call failed inside the fused step loop and left the particle state "
                                          "incomplete; upload x, v and f again (md_upload) before going on");
}

// The sampler `member` of the handle (md_ctx::rdf, dyn, sq, stress; `x` is its name in md_<x>_setup), once its setup has
// succeeded.
template <class S> inline S &sampler_of(md_ctx *ctx, S md_ctx::*member, const char *who, const char *x)
{
    if (ctx->dom.on) throw HipError(std::string(who) + ": not available on a slab-decomposition handle");
    S &s = ctx->*member;
    if (!s.on) throw HipError(std::string(who) + ": no setup (call md_" + x + "_setup first)");
    return s;
}

#define API_BEGIN                                                                                                   \
    if (!ctx) return fail(nullptr, "null handle");                                                                  \
    try {                                                                                                           \
        HIPCHK(hipSetDevice(ctx->device));
#define API_END                                                                                                     \
    }                                                                                                               \
    catch (const std::exception &e) { return fail(ctx, e.what()); }                                                 \
    catch (...) { return fail(ctx, "unknown C++ exception"); }                                                      \
    return 0;

extern "C" {

const char *md_version(void) { return "mdhip 0.1 gfx950"; }

const char *md_last_error(md_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

static int create_common(int dim, int64_t n_global, int64_t n_cap, bool domain, int rank, int nranks,
                         const double *box, double list_cutoff, int device_id, md_ctx **out)
{
    if (!out) return fail(nullptr, "md_create: out is null");
    *out = nullptr;
    if (dim != 2 && dim != 3) return fail(nullptr, "md_create: dim must be 2 or 3");
    if (n_global < 2) return fail(nullptr, "md_create: need at least 2 particles");
    if (n_cap < 2) return fail(nullptr, "md_create: capacity must be at least 2");
    if (n_cap >= (int64_t)MD_VAL_SRC_MASK / 2)
        return fail(nullptr, "md_create: too many particles for one handle (limit 2^25)");
    if (n_global >= (1ll << 31)) return fail(nullptr, "md_create: particle ids must fit 31 bits");
    if (!box) return fail(nullptr, "md_create: box is null");
    if (!(list_cutoff > 0.0)) return fail(nullptr, "md_create: list_cutoff must be positive");
    if (domain && (nranks < 1 || rank < 0 || rank >= nranks))
        return fail(nullptr, "md_create_domain: need nranks >= 1 and 0 <= rank < nranks");
    // the unit cell: column-major d x d, columns = lattice vectors (Julia's Matrix, src/initialization.jl:7-18).  A diagonal
    // matrix takes the orthorhombic fast paths; anything else is a general (triclinic) cell, single handle only.
    CellGeom cg;
    if (const char *why = cell_geometry(dim, box, cg)) return fail(nullptr, why);
    if (cg.tric && domain)
        return fail(nullptr, "md_create_domain: only orthorhombic (diagonal) unit cells are supported by the slab decomposition");
    md_ctx *ctx = nullptr;
    try {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0) return fail(nullptr, "md_create: no HIP device available (libmdhip has no CPU fallback)");
        ctx = new md_ctx();
        if (device_id < 0) HIPCHK(hipGetDevice(&device_id));
        if (device_id >= ndev) throw HipError("md_create: device_id out of range");
        ctx->device = device_id;
        HIPCHK(hipSetDevice(device_id));
        if (domain) {
            // a slab handle's stream carries the collectives and the boundary tiles: the HIGHEST priority, so that the
            // record exchange is not starved of CUs by the interior tiles running beside it on the (lowest-priority)
            // interior stream -- round 2 saw RCCL's copy kernel stretched from 15 to 84 us there
            int plo = 0, phi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&plo, &phi));
            HIPCHK(hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, phi));
        } else {
            HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        }
        ctx->own_stream = ctx->stream;
        ctx->dim = dim;
        ctx->n_global = n_global;
        ctx->ncap = n_cap;
        ctx->n = domain ? 0 : n_cap;
        for (int c = 0; c < dim; ++c) ctx->L[c] = box[c * dim + c];
        ctx->tric = cg.tric;
        for (int c = 0; c < 9; ++c) {
            ctx->A[c] = cg.A[c];
            ctx->Ainv[c] = cg.Ainv[c];
        }
        for (int c = 0; c < 3; ++c) ctx->perp[c] = cg.perp[c];
        ctx->volume = cg.volume;
        ctx->rc = list_cutoff;
        if (domain) {
            ctx->dom.on = true;
            ctx->skin_req = 0.4; // no inner rows on the slab path yet: the single-list optimum
            ctx->dom.rank = rank;
            ctx->dom.nranks = nranks;
            ctx->dom.xlo = ctx->L[0] * rank / nranks;
            ctx->dom.xhi = (rank == nranks - 1) ? ctx->L[0] : ctx->L[0] * (rank + 1) / nranks;
        }
        if (const char *e = getenv("MDHIP_NO_TILES")) ctx->allow_tiles = !(e[0] == '1');
        if (const char *e = getenv("MDHIP_NO_FUSED_BUILD")) ctx->allow_fused_build = !(e[0] == '1');
        if (const char *e = getenv("MDHIP_NO_OWN_FIRST")) ctx->allow_own_first = !(e[0] == '1');
        if (const char *e = getenv("MDHIP_INNER_SKIN")) ctx->inner_skin_req = atof(e);
        if (const char *e = getenv("MDHIP_NO_FUSED_STEP")) ctx->allow_fused = !(e[0] == '1');
        // inner halo (md_kernels.hpp, tile_inner_halo): off unless asked for -- the box test trims only ~4 % of a
        // tile's staged set (tiles straddle bricks; measured) and costs the prune step a block of occupancy
        ctx->allow_inner_halo = false;
        if (const char *e = getenv("MDHIP_INNER_HALO")) ctx->allow_inner_halo = (e[0] == '1');
        // default potential: LennardJones() -- src/potentials.jl:52-64
        ctx->pot_kind = POT_LJ;
        ctx->pp.p[0] = 1.0;
        ctx->pp.p[1] = 1.0;
        ctx->pp.p[2] = 2.5;
        configure_grid(ctx);
        configure_potential(ctx);
        // capacity: owned + ghost shell estimate (self-images, and the neighbours' halo for a slab)
        double frac = 1.0;
        for (int c = 0; c < dim; ++c) frac *= (double)ctx->grid.ncx[c] / ctx->grid.nc[c];
        int64_t gcap = (int64_t)((frac - 1.0) * 1.3 * n_cap) + 4096;
        ctx->cap = n_cap + gcap;
        alloc_state(ctx, 0, ctx->cap);
        alloc_state(ctx, 1, ctx->cap);
        int64_t n = n_cap;
        ctx->nimg.alloc(ctx->cap + 2);
        ctx->img_off.alloc(ctx->cap + 2);
        HIPCHK(hipMemsetAsync(ctx->nimg.p, 0, sizeof(int32_t) * (ctx->cap + 2), ctx->stream));
        ctx->newslot.alloc(ctx->cap + 1);
        ctx->keys_in.alloc(ctx->cap);
        ctx->keys_out.alloc(ctx->cap);
        ctx->vals_in.alloc(ctx->cap);
        ctx->vals_out.alloc(ctx->cap);
        ctx->gsrc.alloc(ctx->cap + 1);
        ctx->gcode.alloc(ctx->cap + 1);
        ctx->gowner.alloc(ctx->cap + 1);
        ctx->nblk = nblocks(ctx->n);
        int nblk_cap = nblocks(n);
        ctx->ntiles = (int64_t)nblk_cap * (MD_BLOCK / 64);
        ctx->nneigh.alloc(n);
        ctx->nmax_tile.alloc(ctx->ntiles);
        // expected neighbours within rc+skin at this density, with headroom
        double dens = (double)n_global;
        dens /= ctx->volume;
        double vol = (dim == 3) ? 4.18879020478639 * ctx->rl * ctx->rl * ctx->rl : 3.14159265358979 * ctx->rl * ctx->rl;
        int maxn = (int)(dens * vol * 1.35) + 24;
        ctx->maxn = (maxn + 3) & ~3;
        ctx->nlist.alloc((size_t)ctx->ntiles * ctx->maxn * 64);
        ctx->nlist16.alloc((size_t)ctx->ntiles * ctx->maxn * 64);
        ctx->halo.alloc((size_t)nblk_cap * ctx->hcap);
        ctx->halo_count.alloc(nblk_cap);
        if (getenv("MDHIP_STAMPS")) ctx->dbg_stamps.alloc((size_t)nblk_cap * 32);
        ctx->partials.alloc((size_t)3 * nblk_cap);
        HIPCHK(hipMemsetAsync(ctx->partials.p, 0, sizeof(double) * 3 * nblk_cap, ctx->stream));
        ctx->scal.alloc(1);
        Scalars h{};
        h.scale = 1.0;
        h.first_viol = MD_NO_VIOLATION;
        HIPCHK(hipMemcpyAsync(ctx->scal.p, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
        ctx->d_kt.alloc(1);
        ctx->d_r1.alloc(1);
        ctx->d_r2.alloc(1);
        if (domain) {
            int64_t rec_cap = n_cap / 2 + 8192;
            ctx->dom.alive.alloc(2 * ctx->cap + 2);
            ctx->dom.counters.alloc(8);
            for (int sd = 0; sd < 2; ++sd) {
                ctx->dom.sbuf[sd].alloc((size_t)rec_cap * MD_MIG_REC);
                ctx->dom.rbuf[sd].alloc((size_t)rec_cap * MD_MIG_REC);
                ctx->dom.hs_src[sd].alloc(rec_cap);
                ctx->dom.send_slot[sd].alloc(rec_cap);
            }
            ctx->dom.xh_slot.alloc(2 * rec_cap);
        }
        for (int w = 0; w < 2; ++w)
            k_init_state<<<nblocks(ctx->cap + 1), MD_BLOCK, 0, ctx->stream>>>((int)n, ctx->cap, ctx->dev(w), dim);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
    } catch (const std::exception &e) {
        g_create_error = e.what();
        delete ctx;
        return 1;
    }
    *out = ctx;
    return 0;
}

int md_create(int dim, int64_t n_particles, const double *box, double list_cutoff, int device_id, md_ctx **out)
{
    return create_common(dim, n_particles, n_particles, false, 0, 1, box, list_cutoff, device_id, out);
}

int md_create_domain(int dim, int64_t n_global, int64_t n_cap, const double *box, double list_cutoff,
                     int device_id, int rank, int nranks, md_ctx **out)
{
    return create_common(dim, n_global, n_cap, true, rank, nranks, box, list_cutoff, device_id, out);
}

static void dom_p2p_teardown(md_ctx *c);

int md_destroy(md_ctx *ctx)
{
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->own_stream);
        if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
        if (ctx->ev_snap_ready) (void)hipEventDestroy(ctx->ev_snap_ready);
        if (ctx->ev_snap_copied) (void)hipEventDestroy(ctx->ev_snap_copied);
        if (ctx->pin_x) (void)hipHostFree(ctx->pin_x);
        if (ctx->pin_i) (void)hipHostFree(ctx->pin_i);
    }
    delete ctx->rtc;
    ctx->rtc = nullptr;
    if (ctx->dom.stream_i) {
        (void)hipStreamSynchronize(ctx->dom.stream_i);
        (void)hipStreamDestroy(ctx->dom.stream_i);
        (void)hipEventDestroy(ctx->dom.ev_go);
        (void)hipEventDestroy(ctx->dom.ev_int);
    }
    dom_p2p_teardown(ctx);
    if (ctx->dom.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->dom.comm);
    ctx->dom.comm = nullptr;
    for (auto &p : ctx->prof_ev) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    delete ctx;
    return 0;
}

int md_set_potential(md_ctx *ctx, int kind, const double *params, int nparams)
{
    API_BEGIN
    if (kind != MD_POT_LJ && kind != MD_POT_PSEUDOHS && kind != MD_POT_POLYDISPERSE && kind != MD_POT_LJ_MODIFIED)
        throw HipError("md_set_potential: unknown potential kind");
    if (nparams < 0 || nparams > 8 || (nparams > 0 && !params)) throw HipError("md_set_potential: bad params");
    int need = (kind == MD_POT_LJ) ? 3 : (kind == MD_POT_PSEUDOHS ? 1 : (kind == MD_POT_LJ_MODIFIED ? 5 : 2));
    if (nparams < need) throw HipError("md_set_potential: too few parameters for this kind");
    // (the LJ kinds' r_cut becomes a threshold on d^2: it has to be a positive finite number)
    if ((kind == MD_POT_LJ || kind == MD_POT_LJ_MODIFIED) && !(std::isfinite(params[2]) && params[2] > 0.0))
        throw HipError("md_set_potential: r_cut must be finite and > 0");
    for (int i = 0; i < 8; ++i) ctx->pp.p[i] = (i < nparams) ? params[i] : 0.0;
    if (kind == MD_POT_LJ_MODIFIED) {
        // the constructor's constants: src/potentials.jl:52-64 (from the struct's sigma and r_cut)
        double eps = params[0], sg = params[1], rc = params[2];
        int mode = (int)params[3];
        if (mode < 0 || mode > 2) throw HipError("md_set_potential: MD_POT_LJ_MODIFIED mode must be 0, 1 or 2");
        if (mode == 2 && !(params[4] < rc)) throw HipError("md_set_potential: XPLOR needs r_on < r_cut");
        double s = sg / rc, s2 = s * s, s6 = s2 * s2 * s2, s12 = s6 * s6;
        ctx->pp.p[5] = 4.0 * eps * (s12 - s6);
        ctx->pp.p[6] = 24.0 * eps * (2.0 * s12 - s6) / rc;
    }
    ctx->pot_kind = kind;
    ctx->list_valid = false; // the LDS record stride of the rows depends on the potential kind
    ctx->hess.frozen = false;
    configure_potential(ctx);
    API_END
}

int md_set_potential_source(md_ctx *ctx, const char *hip_src, const char *entry_name, const double *params,
                            int nparams)
{
    API_BEGIN
    if (!hip_src || !entry_name || !entry_name[0]) throw HipError("md_set_potential_source: source and entry name are required");
    if (nparams < 0 || nparams > 8 || (nparams > 0 && !params)) throw HipError("md_set_potential_source: at most 8 parameters");
    for (const char *q = entry_name; *q; ++q)
        if (!((*q >= 'a' && *q <= 'z') || (*q >= 'A' && *q <= 'Z') || (*q >= '0' && *q <= '9') || *q == '_'))
            throw HipError("md_set_potential_source: entry name must be a plain identifier");
    RtcModule *m = rtc_build(hip_src, entry_name); // throws with the compiler log on error
    delete ctx->rtc;
    ctx->rtc = m;
    for (int i = 0; i < 8; ++i) ctx->pp.p[i] = (i < nparams) ? params[i] : 0.0;
    ctx->pot_kind = POT_CUSTOM;
    ctx->list_valid = false;
    ctx->hess.frozen = false;
    configure_potential(ctx);
    API_END
}

int md_set_skin(md_ctx *ctx, double skin)
{
    API_BEGIN
    if (!(skin >= 0.0)) throw HipError("md_set_skin: skin must be >= 0");
    ctx->skin_req = skin;
    double old_rl = ctx->rl;
    configure_grid(ctx);
    if (ctx->rl > old_rl) {
        double dens = (double)ctx->n_global;
        dens /= ctx->volume;
        double vol = (ctx->dim == 3) ? 4.18879020478639 * ctx->rl * ctx->rl * ctx->rl
                                     : 3.14159265358979 * ctx->rl * ctx->rl;
        int maxn = ((int)(dens * vol * 1.35) + 24 + 3) & ~3;
        if (maxn > ctx->maxn) {
            ctx->maxn = maxn;
            ctx->nlist.alloc((size_t)ctx->ntiles * ctx->maxn * 64);
            ctx->nlist16.alloc((size_t)ctx->ntiles * ctx->maxn * 64);
        }
    }
    ctx->target_interval = 8;
    ctx->rate_known = false;
    API_END
}

int md_set_inner_skin(md_ctx *ctx, double inner_skin)
{
    API_BEGIN
    if (!(inner_skin >= 0.0)) throw HipError("md_set_inner_skin: must be >= 0");
    ctx->inner_skin_req = inner_skin;
    ctx->list_valid = false;
    ctx->rate_known = false;
    API_END
}

int md_upload(md_ctx *ctx, const double *x, const double *v, const double *f, const int32_t *images,
              const double *diameters)
{
    API_BEGIN
    size_t nd = (size_t)ctx->n * ctx->dim;
    hipStream_t st = ctx->stream;
    ctx->hess.frozen = false;
    if (x) {
        ctx->io_x.ensure(nd);
        HIPCHK(hipMemcpyAsync(ctx->io_x.p, x, nd * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (v) {
        ctx->io_v.ensure(nd);
        HIPCHK(hipMemcpyAsync(ctx->io_v.p, v, nd * sizeof(double), hipMemcpyHostToDevice, st));
        ctx->rate_known = false; // new velocities: re-measure the displacement rate the schedule is planned on
    }
    if (f) {
        ctx->io_f.ensure(nd);
        HIPCHK(hipMemcpyAsync(ctx->io_f.p, f, nd * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (images) {
        ctx->io_i.ensure(nd);
        HIPCHK(hipMemcpyAsync(ctx->io_i.p, images, nd * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    if (diameters) {
        ctx->io_d.ensure(ctx->n);
        HIPCHK(hipMemcpyAsync(ctx->io_d.p, diameters, ctx->n * sizeof(double), hipMemcpyHostToDevice, st));
        bool uni = true;
        for (int64_t i = 1; i < ctx->n; ++i)
            if (diameters[i] != diameters[0]) {
                uni = false;
                break;
            }
        ctx->uniform_sigma = uni && !getenv("MDHIP_PROBE_NONUNIFORM"); // (probe: time the 32-byte-record kernels on the bench workload)
        ctx->sigma_u = diameters[0];
        ctx->sigma_max = *std::max_element(diameters, diameters + ctx->n);
        configure_potential(ctx);
    }
    DevState s = ctx->dev(ctx->cur);
    int nb = ctx->nblk;
    if (ctx->dim == 3)
        k_import<3><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, ctx->grid, x ? ctx->io_x.p : nullptr, v ? ctx->io_v.p : nullptr,
                                             f ? ctx->io_f.p : nullptr, images ? ctx->io_i.p : nullptr,
                                             diameters ? ctx->io_d.p : nullptr);
    else
        k_import<2><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, ctx->grid, x ? ctx->io_x.p : nullptr, v ? ctx->io_v.p : nullptr,
                                             f ? ctx->io_f.p : nullptr, images ? ctx->io_i.p : nullptr,
                                             diameters ? ctx->io_d.p : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st)); // host buffers are only borrowed for this call
    if (x || diameters) ctx->list_valid = false;
    if (x) ctx->naff.marked = false; // (md_nonaffine_mark described the frame these positions replace)
    if (x && v && f) {
        // a complete new state: whatever a failed step loop left behind is gone
        ctx->state_invalid = false;
        ctx->fz_a = 0;
    }
    API_END
}

int md_download(md_ctx *ctx, double *x, double *v, double *f, int32_t *images)
{
    API_BEGIN
    require_state(ctx, "md_download");
    size_t nd = (size_t)ctx->n * ctx->dim;
    hipStream_t st = ctx->stream;
    ctx->io_x.ensure(nd);
    ctx->io_v.ensure(nd);
    ctx->io_f.ensure(nd);
    ctx->io_i.ensure(nd);
    DevState s = ctx->dev(ctx->cur);
    int nb = ctx->nblk;
    if (ctx->dim == 3)
        k_export<3><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, ctx->grid, ctx->io_x.p, ctx->io_v.p, ctx->io_f.p, ctx->io_i.p);
    else
        k_export<2><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, ctx->grid, ctx->io_x.p, ctx->io_v.p, ctx->io_f.p, ctx->io_i.p);
    HIPCHK(hipGetLastError());
    if (x) HIPCHK(hipMemcpyAsync(x, ctx->io_x.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (v) HIPCHK(hipMemcpyAsync(v, ctx->io_v.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (f) HIPCHK(hipMemcpyAsync(f, ctx->io_f.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (images) HIPCHK(hipMemcpyAsync(images, ctx->io_i.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

// Frame export at the trajectory cadence (src/simulation.jl:139-171 writes positions + images): the gather runs on the
// handle's stream, the device-to-host copy on a copy stream into pinned memory, and nobody waits -- the caller enqueues the
// next segment (md_run) and collects the frame with md_snapshot_end when it wants to write it.
int md_snapshot_begin(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_snapshot_begin");
    if (ctx->snap_pending) throw HipError("md_snapshot_begin: the previous frame has not been collected (md_snapshot_end)");
    size_t nd = (size_t)ctx->n * ctx->dim;
    hipStream_t st = ctx->stream;
    if (!ctx->copy_stream) {
        HIPCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ctx->ev_snap_ready, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ctx->ev_snap_copied, hipEventDisableTiming));
    }
    if (ctx->pin_n < nd) {
        if (ctx->pin_x) (void)hipHostFree(ctx->pin_x);
        if (ctx->pin_i) (void)hipHostFree(ctx->pin_i);
        ctx->pin_x = nullptr;
        ctx->pin_i = nullptr;
        ctx->pin_n = 0;
        HIPCHK(hipHostMalloc((void **)&ctx->pin_x, nd * sizeof(double), hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void **)&ctx->pin_i, nd * sizeof(int32_t), hipHostMallocDefault));
        ctx->pin_n = nd;
    }
    ctx->snap_x.ensure(nd);
    ctx->snap_i.ensure(nd);
    DevState s = ctx->dev(ctx->cur);
    int nb = ctx->nblk;
    if (ctx->dim == 3)
        k_export<3><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, ctx->grid, ctx->snap_x.p, nullptr, nullptr, ctx->snap_i.p);
    else
        k_export<2><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, ctx->grid, ctx->snap_x.p, nullptr, nullptr, ctx->snap_i.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev_snap_ready, st));
    HIPCHK(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_snap_ready, 0));
    HIPCHK(hipMemcpyAsync(ctx->pin_x, ctx->snap_x.p, nd * sizeof(double), hipMemcpyDeviceToHost, ctx->copy_stream));
    HIPCHK(hipMemcpyAsync(ctx->pin_i, ctx->snap_i.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->copy_stream));
    HIPCHK(hipEventRecord(ctx->ev_snap_copied, ctx->copy_stream));
    ctx->snap_pending = true;
    API_END
}

int md_snapshot_end(md_ctx *ctx, double *x, int32_t *images)
{
    API_BEGIN
    if (!ctx->snap_pending) throw HipError("md_snapshot_end: no frame in flight (md_snapshot_begin first)");
    HIPCHK(hipEventSynchronize(ctx->ev_snap_copied));
    ctx->snap_pending = false;
    size_t nd = (size_t)ctx->n * ctx->dim;
    if (x) memcpy(x, ctx->pin_x, nd * sizeof(double));
    if (images) memcpy(images, ctx->pin_i, nd * sizeof(int32_t));
    API_END
}

int md_compute_forces(md_ctx *ctx, double *energy, double *virial)
{
    API_BEGIN
    require_state(ctx, "md_compute_forces");
    if (!ctx->list_valid) rebuild(ctx);
    launch_force(ctx, true, false, 0.0, -1, 1); // outer rows: always valid for the current positions
    launch_finalize(ctx, true, false, 1.0, 0.0, -1);
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    if (energy) *energy = h.U;
    if (virial) *virial = h.W;
    API_END
}

int md_neighbor_pairs(md_ctx *ctx, int32_t *pairs, int64_t cap, int64_t *count)
{
    API_BEGIN
    require_state(ctx, "md_neighbor_pairs");
    if (cap < 0 || (cap > 0 && !pairs)) throw HipError("md_neighbor_pairs: bad output buffer");
    if (!ctx->list_valid) rebuild(ctx);
    hipStream_t st = ctx->stream;
    DBuf<int32_t> out;
    out.alloc((size_t)std::max<int64_t>(cap, 1) * 2);
    unsigned long long zero = 0;
    HIPCHK(hipMemcpyAsync(&ctx->scal.p->pair_count, &zero, sizeof zero, hipMemcpyHostToDevice, st));
    DevState s = ctx->dev(ctx->cur);
    double c2 = ctx->rc * ctx->rc;
    const uint16_t *l16 = ctx->have_nlist32 ? nullptr : ctx->nlist16.p;
    if (ctx->dim == 3)
        k_pairs<3><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, s, c2, ctx->nlist.p, l16, ctx->tile_rs, ctx->halo.p, ctx->hcap,
                                                   ctx->maxn, ctx->nneigh.p, out.p, (unsigned long long)cap,
                                                   ctx->scal.p);
    else
        k_pairs<2><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, s, c2, ctx->nlist.p, l16, ctx->tile_rs, ctx->halo.p, ctx->hcap,
                                                   ctx->maxn, ctx->nneigh.p, out.p, (unsigned long long)cap,
                                                   ctx->scal.p);
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    int64_t found = (int64_t)h.pair_count;
    if (count) *count = found;
    int64_t ncopy = std::min(found, cap);
    if (ncopy > 0) {
        HIPCHK(hipMemcpyAsync(pairs, out.p, (size_t)ncopy * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    API_END
}

// Instrumentation: the Verlet rows as they are (include/mdhip.h).  Never builds or prunes; reads what the next force
// evaluation would walk (which = 0: outer rows, 1: inner rows) through md_listrows.hpp.
int md_list_rows(md_ctx *ctx, int which, double *info, int32_t *entries, int64_t cap, int64_t *count, double *x0,
                 double *x1, double *pos)
{
    API_BEGIN
    require_state(ctx, "md_list_rows");
    if (ctx->dom.on) throw HipError("md_list_rows: not available on a slab-decomposition handle");
    if (which != 0 && which != 1) throw HipError("md_list_rows: which must be 0 (outer rows) or 1 (inner rows)");
    if (cap < 0 || (cap > 0 && !entries)) throw HipError("md_list_rows: bad output buffer");
    if ((x0 || x1 || pos) && !(x0 && x1 && pos)) throw HipError("md_list_rows: x0, x1 and pos are given together or not at all");
    hipStream_t st = ctx->stream;
    const int n = (int)ctx->n;
    const bool valid = ctx->list_valid;
    const bool inner = valid && ctx->inner_valid;
    if (which == 1 && !inner) throw HipError("md_list_rows: no valid inner rows (inner_valid = 0)");
    if (info) {
        double d1 = 0.0;
        if (inner) {
            Scalars h = read_scalars(ctx);
            unsigned long long bits = h.d1max2_bits;
            double d12;
            memcpy(&d12, &bits, sizeof d12);
            d1 = std::sqrt(d12);
        }
        // (after md_scale_cell: what the kept rows still cover -- the effective skin, list radius and inner skin; d1 was
        // scaled on the device)
        const double v[MD_LIST_ROWS_INFO] = {ctx->rc, valid ? skin_eff(ctx) : ctx->skin, valid ? rl_eff(ctx) : ctx->rl,
                                             inner ? inner_eff(ctx) : 0.0, d1,
                                             valid ? 1.0 : 0.0, inner ? 1.0 : 0.0, (valid && ctx->use_tiles) ? 1.0 : 0.0,
                                             (valid && ctx->use_tiles && !ctx->have_nlist32) ? 1.0 : 0.0,
                                             (valid && ctx->own_first) ? 1.0 : 0.0,
                                             (inner && ctx->inner_halo_live) ? 1.0 : 0.0, (double)ctx->n,
                                             (valid && !ctx->use_tiles) ? 1.0 : 0.0, (double)ctx->nghost,
                                             (valid && ctx->virtual_ghosts) ? 1.0 : 0.0, (valid && ctx->prune_on) ? 1.0 : 0.0};
        memcpy(info, v, sizeof v);
    }
    DevState s = ctx->dev(ctx->cur);
    if (pos && n > 0) {
        const size_t nd = (size_t)n * ctx->dim;
        DBuf<double> o;
        o.alloc(3 * nd);
        if (ctx->dim == 3)
            k_listrows_positions<3><<<ctx->nblk, MD_BLOCK, 0, st>>>(n, s, o.p, o.p + nd, o.p + 2 * nd);
        else
            k_listrows_positions<2><<<ctx->nblk, MD_BLOCK, 0, st>>>(n, s, o.p, o.p + nd, o.p + 2 * nd);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(x0, o.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(x1, o.p + nd, nd * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(pos, o.p + 2 * nd, nd * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    int64_t total = 0;
    if (valid && n > 0) {
        ListRowsView V{};
        V.n = n;
        V.nghost = (int)ctx->nghost;
        V.id = s.id;
        V.maxn = ctx->maxn;
        V.sentinel32 = (uint32_t)ctx->cap;
        V.gowner = ctx->gowner.p;
        V.gcode = ctx->gcode.p;
        if (ctx->use_tiles) {
            const bool hin = which == 1 && ctx->inner_halo_live;
            V.rows16 = which == 1 ? ctx->nlist16_in.p : ctx->nlist16.p;
            V.rowlen = which == 1 ? ctx->nmax_tile_in.p : ctx->nmax_tile.p;
            V.rs = ctx->tile_rs;
            V.halo = hin ? ctx->halo_in.p : ctx->halo.p;
            V.hcap = hin ? ctx->hcap_in : ctx->hcap;
            V.halo_count = hin ? ctx->halo_in_count.p : ctx->halo_count.p;
        } else {
            V.rows32 = ctx->nlist.p;
            V.rowlen = ctx->nmax_tile.p;
        }
        DBuf<int32_t> cnt;
        cnt.alloc((size_t)n);
        k_listrows<false><<<ctx->nblk, MD_BLOCK, 0, st>>>(V, cnt.p, nullptr, nullptr, 0);
        HIPCHK(hipGetLastError());
        std::vector<int32_t> hc((size_t)n);
        HIPCHK(hipMemcpyAsync(hc.data(), cnt.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<int64_t> off((size_t)n);
        for (int k = 0; k < n; ++k) {
            off[k] = total;
            total += hc[k];
        }
        const int64_t ncopy = std::min(total, cap);
        if (ncopy > 0) {
            DBuf<int64_t> doff;
            doff.alloc((size_t)n);
            DBuf<int32_t> out;
            out.alloc((size_t)ncopy * 5);
            HIPCHK(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
            k_listrows<true><<<ctx->nblk, MD_BLOCK, 0, st>>>(V, nullptr, doff.p, out.p, (long long)ncopy);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(entries, out.p, (size_t)ncopy * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    if (count) *count = total;
    API_END
}

// ---------------------------------------------------------------------------------------------
// Shared by the sampler entry points below, with sampler_of above: the argument checks here; for the four samplers that
// correlate the current frame with stored origins (md_dyn_*, md_sq_*, md_cage_*, md_chi4_*, md_cur_*) also SlotRows and
// alloc_or_refuse at the top of this file and dyn_zero / sq_zero / cage_zero / chi4_zero / cur_zero, dyn_params,
// batch_from and for_batches above; for the three that sum over wave vectors (md_sq_*, md_chi4_*, md_cur_*) ModeSet.
static void check_range(const char *who, const char *name, int v, int lo, int hi)
{
    if (v >= lo && v <= hi) return;
    char b[200];
    snprintf(b, sizeof b, "%s: %s must be in %d..%d, got %d", who, name, lo, hi, v);
    throw HipError(b);
}

// Squared bin edges e2[k] = (k delta)^2, delta = r_max / nbins, k = 0..nbins: the table decides every bin of the g(r)
// and the van Hove histograms.  All zeros when nbins == 0.
static std::vector<double> squared_edges(double r_max, int nbins)
{
#pragma clang fp contract(off)
    std::vector<double> e2(nbins + 1, 0.0);
    if (nbins > 0) {
        const double delta = r_max / nbins;
        for (int k = 0; k <= nbins; ++k) {
            double rk = (double)k * delta;
            e2[k] = rk * rk;
        }
    }
    return e2;
}

static void check_nrows(const char *who, int nrows, int lo)
{
    if (nrows >= lo) return;
    char b[200];
    snprintf(b, sizeof b, "%s: nrows must be >= %d, got %d", who, lo, nrows);
    throw HipError(b);
}

// The wave numbers of md_dyn_setup / md_cage_setup
static void check_q(const char *who, const double *q, int nq)
{
    check_range(who, "nq", nq, 0, MD_DYN_MAX_Q);
    if (nq > 0 && !q) throw HipError(std::string(who) + ": q is null");
    for (int j = 0; j < nq; ++j)
        if (!std::isfinite(q[j])) {
            char b[200];
            snprintf(b, sizeof b, "%s: q[%d] must be finite", who, j);
            throw HipError(b);
        }
}

// The integer wave vectors of md_sq_setup / md_chi4_setup, nvec x dim: every component in range, none of them n = 0
// (`zero_hint` says why that one is refused)
static void check_wave_vectors(const char *who, const int32_t *nvecs, int nvec, int dim, const char *zero_hint)
{
    char b[240];
    for (int v = 0; v < nvec; ++v) {
        bool zero = true;
        for (int c = 0; c < dim; ++c) {
            const int32_t k = nvecs[(size_t)v * dim + c];
            if (k < -MD_SQ_MAX_N || k > MD_SQ_MAX_N) {
                snprintf(b, sizeof b, "%s: component %d of vector %d is %d, outside -%d..%d", who, c, v, (int)k, MD_SQ_MAX_N,
                         MD_SQ_MAX_N);
                throw HipError(b);
            }
            zero = zero && k == 0;
        }
        if (zero) {
            snprintf(b, sizeof b, "%s: vector %d is n = 0 (%s)", who, v, zero_hint);
            throw HipError(b);
        }
    }
}

// The gather md_download makes, of the wrapped coordinates and image counts -- and, with v, the velocities -- into a
// sampler's own frame buffers.
static void export_frame(md_ctx *ctx, double *x, int32_t *im, double *v = nullptr)
{
    DevState s = ctx->dev(ctx->cur);
    if (ctx->dim == 3)
        k_export<3><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, ctx->grid, x, v, nullptr, im);
    else
        k_export<2><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, ctx->grid, x, v, nullptr, im);
    HIPCHK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// Radial distribution function (md_rdf.hpp): a sample reads the state and writes only the rdf scratch, so the step
// loop, the list and the cell order are exactly what they would have been without it.
// The cell grid of a pair walk out to r_max (md_rdf_*, md_mpc_*), after the face-distance rule: cells at least r_max
// wide between their faces (fractional cut, as configure_grid does for the list), at least 3 per direction (every pair
// within r_max is then visited once, with its minimum image); no more cells than about two per particle -- wider cells
// are still correct, only the walk grows.
static RdfGrid pair_walk_grid(md_ctx *ctx, const char *who, double r_max)
{
    for (int c = 0; c < ctx->dim; ++c)
        if (ctx->perp[c] < 3.0 * r_max) {
            char b[320];
            snprintf(b, sizeof b,
                     "%s: r_max = %.17g is too large: the face distance %.17g of lattice direction %d must be "
                     ">= 3*r_max (limit r_max <= %.17g)",
                     who, r_max, ctx->perp[c], c, ctx->perp[c] / 3.0);
            throw HipError(b);
        }
    RdfGrid g{};
    const int64_t n = ctx->n;
    for (int c = 0; c < 3; ++c) {
        g.nc[c] = 1;
        if (c >= ctx->dim) continue;
        int k = (int)std::min(std::floor(ctx->perp[c] / r_max), 4096.0);
        while (k > 3 && ctx->perp[c] / k < r_max) --k;
        g.nc[c] = std::max(k, 3);
    }
    auto ncells = [&] { return (int64_t)g.nc[0] * g.nc[1] * g.nc[2]; };
    const int64_t cell_cap = std::max<int64_t>(2 * n, 27);
    while (ncells() > cell_cap) {
        int c = 0;
        for (int d = 1; d < ctx->dim; ++d)
            if (g.nc[d] > g.nc[c]) c = d;
        if (g.nc[c] <= 3) break;
        --g.nc[c];
    }
    g.ncell = (int)ncells();
    for (int c = 0; c < 9; ++c) {
        g.A[c] = ctx->A[c];
        g.Ainv[c] = ctx->Ainv[c];
    }
    return g;
}

int md_rdf_setup(md_ctx *ctx, double r_max, int nbins)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_rdf_setup: not available on a slab-decomposition handle");
    if (!(r_max > 0.0) || !std::isfinite(r_max)) throw HipError("md_rdf_setup: r_max must be finite and > 0");
    check_range("md_rdf_setup", "nbins", nbins, 1, MD_RDF_MAX_BINS);
    const RdfGrid grid = pair_walk_grid(ctx, "md_rdf_setup", r_max);
    md_ctx::Rdf &R = ctx->rdf;
    R.on = false;
    RdfGrid &g = R.grid;
    g = grid;
    const int64_t n = ctx->n;
    const std::vector<double> e2 = squared_edges(r_max, nbins);
    hipStream_t st = ctx->stream;
    R.e2.alloc(nbins + 1);
    R.hist.alloc(nbins);
    R.wrec.alloc(n);
    R.srec.alloc(n);
    R.keys_in.alloc(n);
    R.keys_out.alloc(n);
    R.vals_in.alloc(n);
    R.vals_out.alloc(n);
    R.cell_start.alloc((size_t)g.ncell + 1);
    R.cell_end.alloc((size_t)g.ncell + 1);
    R.work.alloc(1);
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, R.keys_in.p, R.keys_out.p, R.vals_in.p, R.vals_out.p, (size_t)n,
                                     0u, (unsigned)std::max(1, ceil_log2((uint64_t)g.ncell)), st));
    R.sort_tmp.alloc(tmp_bytes);
    HIPCHK(hipMemcpyAsync(R.e2.p, e2.data(), sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(R.hist.p, 0, sizeof(unsigned long long) * nbins, st));
    size_t lds = sizeof(double) * (nbins + 1) + sizeof(uint32_t) * nbins;
    if (ctx->dim == 3)
        HIPCHK(hipFuncSetAttribute((const void *)k_rdf_hist<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    else
        HIPCHK(hipFuncSetAttribute((const void *)k_rdf_hist<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipStreamSynchronize(st)); // (the edge table is a host vector)
    R.r_max = r_max;
    R.nbins = nbins;
    R.nsamples = 0;
    R.on = true;
    API_END
}

int md_rdf_sample(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_rdf_sample");
    md_ctx::Rdf &R = sampler_of(ctx, &md_ctx::rdf, "md_rdf_sample", "rdf");
    const int n = (int)ctx->n;
    const RdfGrid &g = R.grid;
    hipStream_t st = ctx->stream;
    DevState s = ctx->dev(ctx->cur);
    if (ctx->dim == 3)
        k_rdf_key<3><<<nblocks(n), MD_BLOCK, 0, st>>>(n, s, ctx->grid, g, R.wrec.p, R.keys_in.p, R.vals_in.p);
    else
        k_rdf_key<2><<<nblocks(n), MD_BLOCK, 0, st>>>(n, s, ctx->grid, g, R.wrec.p, R.keys_in.p, R.vals_in.p);
    HIPCHK(hipGetLastError());
    size_t tmp_bytes = R.sort_tmp.n;
    HIPCHK(rocprim::radix_sort_pairs(R.sort_tmp.p, tmp_bytes, R.keys_in.p, R.keys_out.p, R.vals_in.p, R.vals_out.p,
                                     (size_t)n, 0u, (unsigned)std::max(1, ceil_log2((uint64_t)g.ncell)), st));
    HIPCHK(hipMemsetAsync(R.cell_start.p, 0, sizeof(int32_t) * (g.ncell + 1), st));
    HIPCHK(hipMemsetAsync(R.cell_end.p, 0, sizeof(int32_t) * (g.ncell + 1), st));
    HIPCHK(hipMemsetAsync(R.work.p, 0, sizeof(int32_t), st));
    k_rdf_gather<<<nblocks(n), MD_BLOCK, 0, st>>>(n, R.keys_out.p, R.vals_out.p, R.wrec.p, R.srec.p, R.cell_start.p,
                                                  R.cell_end.p);
    HIPCHK(hipGetLastError());
    // one wave per home cell at a time, cells handed out by the work counter; the grid only needs to fill the chip
    const int waves_per_block = MD_RDF_BLOCK / 64;
    const int nblk = (int)std::min<int64_t>((g.ncell + waves_per_block - 1) / waves_per_block, 1024);
    const size_t lds = sizeof(double) * (R.nbins + 1) + sizeof(uint32_t) * R.nbins;
    const float inv_delta = (float)(R.nbins / R.r_max);
    if (ctx->dim == 3)
        k_rdf_hist<3><<<nblk, MD_RDF_BLOCK, lds, st>>>(g, R.nbins, inv_delta, R.e2.p, R.srec.p, R.cell_start.p,
                                                      R.cell_end.p, R.work.p, R.hist.p);
    else
        k_rdf_hist<2><<<nblk, MD_RDF_BLOCK, lds, st>>>(g, R.nbins, inv_delta, R.e2.p, R.srec.p, R.cell_start.p,
                                                      R.cell_end.p, R.work.p, R.hist.p);
    HIPCHK(hipGetLastError());
    ++R.nsamples;
    API_END
}

int md_rdf_read(md_ctx *ctx, int64_t *counts, int64_t *nsamples)
{
    API_BEGIN
    md_ctx::Rdf &R = sampler_of(ctx, &md_ctx::rdf, "md_rdf_read", "rdf");
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the device words are read back as int64_t");
    if (counts) HIPCHK(hipMemcpyAsync(counts, R.hist.p, sizeof(int64_t) * R.nbins, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (nsamples) *nsamples = R.nsamples;
    API_END
}

int md_rdf_reset(md_ctx *ctx)
{
    API_BEGIN
    md_ctx::Rdf &R = sampler_of(ctx, &md_ctx::rdf, "md_rdf_reset", "rdf");
    HIPCHK(hipMemsetAsync(R.hist.p, 0, sizeof(unsigned long long) * R.nbins, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    R.nsamples = 0;
    API_END
}

// ---------------------------------------------------------------------------------------------
// Self dynamics (md_dyn.hpp): an origin store and a sample each launch k_export -- the gather md_download makes -- into the
// sampler's own buffers and read nothing else of the state, so the step loop, the list and the cell order are exactly
// what they would have been without them.
int md_dyn_setup(md_ctx *ctx, int nslots, int nrows, const double *q, int nq, double r_max, int nbins)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_dyn_setup: not available on a slab-decomposition handle");
    char b[320];
    check_range("md_dyn_setup", "nslots", nslots, 1, MD_DYN_MAX_SLOTS);
    check_nrows("md_dyn_setup", nrows, 1);
    check_q("md_dyn_setup", q, nq);
    check_range("md_dyn_setup", "nbins", nbins, 0, MD_DYN_MAX_BINS);
    if (nbins > 0 && (!(r_max > 0.0) || !std::isfinite(r_max)))
        throw HipError("md_dyn_setup: r_max must be finite and > 0 when nbins > 0");
    md_ctx::Dyn &Y = ctx->dyn;
    Y.on = false;
    const int64_t n = ctx->n;
    const size_t frame = (size_t)n * ctx->dim;
    // MDHIP_DYN_ALLOC_LIMIT=bytes refuses origin slots above this size
    snprintf(b, sizeof b, "%d origin slots (nslots*N*d*12 = %d*%lld*%d*12)", nslots, nslots, (long long)n, ctx->dim);
    alloc_or_refuse("md_dyn_setup", "MDHIP_DYN_ALLOC_LIMIT", (size_t)nslots * frame * 12, b,
                    std::make_pair(&Y.ox, (size_t)nslots * frame), std::make_pair(&Y.oi, (size_t)nslots * frame));
    const int nquant = 2 + nq;
    Y.cx.alloc(frame);
    Y.ci.alloc(frame);
    Y.part.alloc((size_t)MD_DYN_MAX_BATCH * nquant * blocks_of(n, MD_DYN_BLOCK * MD_DYN_PPT));
    Y.sums.alloc((size_t)nrows * nquant);
    Y.hist.alloc((size_t)nrows * std::max(nbins, 1));
    Y.e2.alloc((size_t)nbins + 1);
    const std::vector<double> e2 = squared_edges(r_max, nbins);
    HIPCHK(hipMemcpyAsync(Y.e2.p, e2.data(), sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, ctx->stream));
    Y.sr.init(nslots, nrows);
    Y.nq = nq;
    Y.nbins = nbins;
    Y.r_max = nbins > 0 ? r_max : 0.0;
    Y.q.assign(q, q + nq);
    dyn_zero(ctx); // (waits: the edge table is a host vector)
    Y.on = true;
    API_END
}

int md_dyn_origin(md_ctx *ctx, int slot)
{
    API_BEGIN
    md_ctx::Dyn &Y = sampler_of(ctx, &md_ctx::dyn, "md_dyn_origin", "dyn");
    require_state(ctx, "md_dyn_origin");
    Y.sr.check_slot("md_dyn_origin", slot);
    const size_t frame = (size_t)ctx->n * ctx->dim;
    export_frame(ctx, Y.ox.p + (size_t)slot * frame, Y.oi.p + (size_t)slot * frame);
    Y.sr.filled[slot] = 1;
    API_END
}

int md_dyn_sample(md_ctx *ctx, const int32_t *slots, const int32_t *rows, int count)
{
    API_BEGIN
    md_ctx::Dyn &Y = sampler_of(ctx, &md_ctx::dyn, "md_dyn_sample", "dyn");
    require_state(ctx, "md_dyn_sample");
    Y.sr.check_batch("md_dyn_sample", slots, rows, count, "store an origin with md_dyn_origin first");
    if (count == 0) return 0;
    hipStream_t st = ctx->stream;
    export_frame(ctx, Y.cx.p, Y.ci.p);
    const DynParams P = dyn_params(ctx, &Y.q, Y.nbins, Y.r_max);
    const size_t lds = sizeof(uint32_t) * Y.nbins;
    for (int i0 = 0; i0 < count; i0 += MD_DYN_MAX_BATCH) {
        const DynBatch B = batch_from<DynBatch>(slots, rows, i0, count, MD_DYN_MAX_BATCH);
        dim3 grid(P.nblk, B.count);
        if (ctx->dim == 3)
            k_dyn_sample<3><<<grid, MD_DYN_BLOCK, lds, st>>>(P, B, Y.cx.p, Y.ci.p, Y.ox.p, Y.oi.p, Y.e2.p, Y.part.p, Y.hist.p);
        else
            k_dyn_sample<2><<<grid, MD_DYN_BLOCK, lds, st>>>(P, B, Y.cx.p, Y.ci.p, Y.ox.p, Y.oi.p, Y.e2.p, Y.part.p, Y.hist.p);
        HIPCHK(hipGetLastError());
        k_dyn_reduce<<<1, MD_DYN_REDUCE_BLOCK, 0, st>>>(P, B, Y.part.p, Y.sums.p);
        HIPCHK(hipGetLastError());
        Y.sr.count_rows(B.row, B.count);
    }
    API_END
}

int md_dyn_read(md_ctx *ctx, int64_t *nsamples, double *sums, int64_t *hist)
{
    API_BEGIN
    md_ctx::Dyn &Y = sampler_of(ctx, &md_ctx::dyn, "md_dyn_read", "dyn");
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the device words are read back as int64_t");
    const size_t ns = (size_t)Y.sr.nrows * (2 + Y.nq), nh = (size_t)Y.sr.nrows * Y.nbins;
    hipStream_t st = ctx->stream;
    if (sums) HIPCHK(hipMemcpyAsync(sums, Y.sums.p, sizeof(double) * ns, hipMemcpyDeviceToHost, st));
    if (hist && nh) HIPCHK(hipMemcpyAsync(hist, Y.hist.p, sizeof(int64_t) * nh, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    Y.sr.read_counts(nsamples);
    API_END
}

int md_dyn_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::dyn, "md_dyn_reset", "dyn");
    dyn_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Density modes, S(q) and coherent F(q, t) (md_sq.hpp): a sample launches k_export into the sampler's own frame buffer and
// reads nothing else of the state, so the step loop, the list and the cell order are what they would have been without it.
// k_sq_frac of the frame x (n x dim, particle-id order): f = U^-1 x into fr, one array per axis (md_chi4_origin and
// md_cur_sample launch it too; it stands here so that the kernels are emitted where they were)
static void launch_frac(md_ctx *ctx, const double *x, double *fr)
{
    const int n = (int)ctx->n;
    if (ctx->dim == 3)
        k_sq_frac<3><<<nblocks(n), MD_BLOCK, 0, ctx->stream>>>(n, ctx->grid, x, fr);
    else
        k_sq_frac<2><<<nblocks(n), MD_BLOCK, 0, ctx->stream>>>(n, ctx->grid, x, fr);
    HIPCHK(hipGetLastError());
}

int md_sq_setup(md_ctx *ctx, const int32_t *nvecs, int nvec, int nslots, int nrows)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_sq_setup: not available on a slab-decomposition handle");
    check_range("md_sq_setup", "nvec", nvec, 1, MD_SQ_MAX_VEC);
    if (!nvecs) throw HipError("md_sq_setup: n is null");
    check_range("md_sq_setup", "nslots", nslots, 0, MD_SQ_MAX_SLOTS);
    check_nrows("md_sq_setup", nrows, 0);
    const int dim = ctx->dim;
    check_wave_vectors("md_sq_setup", nvecs, nvec, dim, "rho(0) = N carries no information");
    md_ctx::Sq &S = ctx->sq;
    S.on = false;
    const int64_t n = ctx->n;
    const size_t frame = (size_t)n * dim;
    hipStream_t st = ctx->stream;
    S.init(nvecs, nvec, dim, n, 2, st);
    S.cx.alloc(frame);
    S.ci.alloc(frame);
    S.fr.alloc(frame);
    S.rho.alloc((size_t)nvec * 2);
    S.s2.alloc(nvec);
    S.corr.alloc((size_t)nrows * nvec);
    S.org.alloc((size_t)nslots * nvec * 2);
    HIPCHK(hipMemsetAsync(S.rho.p, 0, sizeof(double) * nvec * 2, st));
    if (nslots) HIPCHK(hipMemsetAsync(S.org.p, 0, sizeof(double) * nslots * nvec * 2, st));
    S.sr.init(nslots, nrows);
    S.sampled = false;
    sq_zero(ctx); // (waits)
    S.on = true;
    API_END
}

int md_sq_sample(md_ctx *ctx, int add_static, const int32_t *slots, const int32_t *rows, int count, int origin_slot)
{
    API_BEGIN
    md_ctx::Sq &S = sampler_of(ctx, &md_ctx::sq, "md_sq_sample", "sq");
    require_state(ctx, "md_sq_sample");
    S.sr.check_batch("md_sq_sample", slots, rows, count, "store an origin with origin_slot first");
    S.sr.check_origin("md_sq_sample", origin_slot);
    hipStream_t st = ctx->stream;
    const int n = (int)ctx->n;
    export_frame(ctx, S.cx.p, S.ci.p);
    launch_frac(ctx, S.cx.p, S.fr.p);
    if (ctx->dim == 3)
        k_sq_rho<3><<<dim3(S.nblk, S.nvec_pad / MD_SQ_TILE), MD_SQ_BLOCK, 0, st>>>(n, S.nblk, S.fr.p, S.nd.p, S.part.p);
    else
        k_sq_rho<2><<<dim3(S.nblk, S.nvec_pad / MD_SQ_TILE), MD_SQ_BLOCK, 0, st>>>(n, S.nblk, S.fr.p, S.nd.p, S.part.p);
    HIPCHK(hipGetLastError());
    const int rblk = (S.nvec + MD_SQ_REDUCE_BLOCK / 64 - 1) / (MD_SQ_REDUCE_BLOCK / 64);
    for_batches<SqBatch>(slots, rows, count, MD_SQ_MAX_BATCH, [&](const SqBatch &B, bool first, bool last) {
        k_sq_reduce<<<rblk, MD_SQ_REDUCE_BLOCK, 0, st>>>(S.nvec, S.nblk, first, add_static != 0, B, last ? origin_slot : -1,
                                                        S.part.p, S.rho.p, S.s2.p, S.corr.p, S.org.p);
        HIPCHK(hipGetLastError());
    });
    S.sampled = true;
    if (add_static) ++S.nstatic;
    S.sr.count_rows(rows, count);
    if (origin_slot >= 0) S.sr.filled[origin_slot] = 1;
    API_END
}

int md_sq_rho(md_ctx *ctx, double *rho)
{
    API_BEGIN
    md_ctx::Sq &S = sampler_of(ctx, &md_ctx::sq, "md_sq_rho", "sq");
    if (!S.sampled) throw HipError("md_sq_rho: no frame has been sampled since md_sq_setup");
    if (!rho) throw HipError("md_sq_rho: rho is null");
    HIPCHK(hipMemcpyAsync(rho, S.rho.p, sizeof(double) * S.nvec * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    API_END
}

int md_sq_read(md_ctx *ctx, int64_t *nstatic, double *s2, int64_t *nsamples, double *corr)
{
    API_BEGIN
    md_ctx::Sq &S = sampler_of(ctx, &md_ctx::sq, "md_sq_read", "sq");
    hipStream_t st = ctx->stream;
    if (s2) HIPCHK(hipMemcpyAsync(s2, S.s2.p, sizeof(double) * S.nvec, hipMemcpyDeviceToHost, st));
    if (corr && S.sr.nrows)
        HIPCHK(hipMemcpyAsync(corr, S.corr.p, sizeof(double) * S.sr.nrows * S.nvec, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nstatic) *nstatic = S.nstatic;
    S.sr.read_counts(nsamples);
    API_END
}

int md_sq_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::sq, "md_sq_reset", "sq");
    sq_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Pressure tensor and its lag correlations (md_stress.hpp): a sample walks the OUTER rows -- valid for the current
// positions whenever the list is, as md_compute_forces relies on -- reads positions and velocities and writes only the
// sampler's own buffers, so the step loop, the list and the cell order are exactly what they would have been without it.
int md_stress_setup(md_ctx *ctx, int nlags)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_stress_setup: not available on a slab-decomposition handle");
    if (ctx->pot_kind == POT_CUSTOM) throw HipError("md_stress_setup: not available with a user potential (MD_POT_CUSTOM)");
    check_range("md_stress_setup", "nlags", nlags, 0, MD_STRESS_MAX_LAGS);
    md_ctx::Stress &S = ctx->stress;
    S.on = false;
    const int nc = stress_nc(ctx);
    S.part.alloc((size_t)2 * nc * std::max(nblocks(ctx->n), 1));
    S.last.alloc(2 * nc);
    S.sums.alloc(2 * nc);
    S.ring.alloc((size_t)std::max(nlags, 1) * nc);
    S.corr.alloc((size_t)std::max(nlags, 1) * nc);
    S.nlags = nlags;
    S.sampled = false;
    HIPCHK(hipMemsetAsync(S.last.p, 0, sizeof(double) * 2 * nc, ctx->stream));
    stress_zero(ctx);
    S.on = true;
    API_END
}

int md_stress_sample(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_stress_sample");
    md_ctx::Stress &S = sampler_of(ctx, &md_ctx::stress, "md_stress_sample", "stress");
    if (ctx->pot_kind == POT_CUSTOM) throw HipError("md_stress_sample: not available with a user potential (MD_POT_CUSTOM)");
    if (!ctx->list_valid) rebuild(ctx); // the build md_compute_forces / md_run would make at these positions
    const int nc = stress_nc(ctx);
    S.part.ensure((size_t)2 * nc * std::max(ctx->nblk, 1));
    if (ctx->dim == 3) {
        launch_stress_d<3>(ctx);
        k_stress_finish<3><<<1, 1024, 0, ctx->stream>>>(ctx->nblk, S.part.p, (long long)S.nsamples, S.nlags, S.last.p,
                                                        S.sums.p, S.ring.p, S.corr.p);
    } else {
        launch_stress_d<2>(ctx);
        k_stress_finish<2><<<1, 1024, 0, ctx->stream>>>(ctx->nblk, S.part.p, (long long)S.nsamples, S.nlags, S.last.p,
                                                        S.sums.p, S.ring.p, S.corr.p);
    }
    HIPCHK(hipGetLastError());
    ++S.nsamples;
    S.sampled = true;
    API_END
}

int md_stress_tensor(md_ctx *ctx, double *kin, double *vir)
{
    API_BEGIN
    md_ctx::Stress &S = sampler_of(ctx, &md_ctx::stress, "md_stress_tensor", "stress");
    if (!S.sampled) throw HipError("md_stress_tensor: no frame sampled yet (call md_stress_sample first)");
    const int nc = stress_nc(ctx);
    double h[12];
    HIPCHK(hipMemcpyAsync(h, S.last.p, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < nc; ++c) {
        if (kin) kin[c] = h[c];
        if (vir) vir[c] = h[nc + c];
    }
    API_END
}

int md_stress_read(md_ctx *ctx, int64_t *nsamples, double *sum_kin, double *sum_vir, int64_t *ncorr, double *corr)
{
    API_BEGIN
    md_ctx::Stress &S = sampler_of(ctx, &md_ctx::stress, "md_stress_read", "stress");
    const int nc = stress_nc(ctx);
    double h[12];
    HIPCHK(hipMemcpyAsync(h, S.sums.p, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, ctx->stream));
    if (corr && S.nlags > 0)
        HIPCHK(hipMemcpyAsync(corr, S.corr.p, sizeof(double) * (size_t)S.nlags * nc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (nsamples) *nsamples = S.nsamples;
    for (int c = 0; c < nc; ++c) {
        if (sum_kin) sum_kin[c] = h[c];
        if (sum_vir) sum_vir[c] = h[nc + c];
    }
    // lag k has one product per sample m >= k
    if (ncorr)
        for (int k = 0; k < S.nlags; ++k) ncorr[k] = std::max<int64_t>(S.nsamples - k, 0);
    API_END
}

int md_stress_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::stress, "md_stress_reset", "stress");
    stress_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Bond-orientational order (md_boo.hpp): a sample walks the OUTER rows as md_stress_sample does, never evaluates the
// potential -- so it serves every potential, a user's included -- reads positions only and writes only the sampler's own
// buffers.
int md_boo_setup(md_ctx *ctx, double r_neigh, int order, int nbins, double threshold, int min_conn, int64_t nseries)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_boo_setup: not available on a slab-decomposition handle");
    if (!(r_neigh > 0.0) || !std::isfinite(r_neigh)) throw HipError("md_boo_setup: r_neigh must be finite and > 0");
    if (r_neigh > ctx->rc) {
        char b[256];
        snprintf(b, sizeof b, "md_boo_setup: r_neigh = %.17g exceeds the list cutoff %.17g (the rows are complete only up to it)",
                 r_neigh, ctx->rc);
        throw HipError(b);
    }
    if (ctx->dim == 3) {
        if (order != 4 && order != 6) throw HipError("md_boo_setup: order (l) must be 4 or 6 in 3-D");
    } else {
        check_range("md_boo_setup", "order (k)", order, 1, 12);
    }
    check_range("md_boo_setup", "nbins", nbins, 1, MD_BOO_MAX_BINS);
    check_range("md_boo_setup", "min_conn", min_conn, 0, MD_BOO_NCLAMP);
    if (!std::isfinite(threshold)) throw HipError("md_boo_setup: threshold must be finite");
    if (nseries < 0 || nseries > MD_BOO_MAX_SERIES) throw HipError("md_boo_setup: nseries must be in 0..1048576");
    md_ctx::Boo &B = ctx->boo;
    B.on = false;
    B.sampled = false;
    B.order = order;
    B.nm = ctx->dim == 3 ? order + 1 : 1;
    B.nbins = nbins;
    B.min_conn = min_conn;
    B.threshold = threshold;
    B.rn = r_neigh;
    B.rn2 = r_neigh * r_neigh;
    B.nseries = nseries;
    B.coef = boo_coef(ctx->dim, order);
    const size_t n = (size_t)ctx->n;
    B.qlm.alloc(2 * (size_t)B.nm * n);
    B.norm.alloc(n);
    B.q.alloc(n);
    B.qbar.alloc(n);
    B.nnb.alloc(n);
    B.nconn.alloc(n);
    B.part.alloc((size_t)(7 + 2 * B.nm) * std::max(nblocks(ctx->n), 1));
    B.sum_fr.alloc(MD_BOO_NFR);
    B.series.alloc((size_t)MD_BOO_NFR * std::max<int64_t>(nseries, 1));
    B.hist.alloc(B.nhist());
    B.ids.alloc(n);
    boo_zero(ctx);
    B.on = true;
    API_END
}

int md_boo_sample(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_boo_sample");
    md_ctx::Boo &B = sampler_of(ctx, &md_ctx::boo, "md_boo_sample", "boo");
    if (!ctx->list_valid) rebuild(ctx); // the build md_compute_forces / md_run would make at these positions
    if (ctx->dim == 3) {
        if (B.order == 4)
            launch_boo<3, 4>(ctx);
        else
            launch_boo<3, 6>(ctx);
    } else {
        launch_boo<2, 0>(ctx);
    }
    HIPCHK(hipGetLastError());
    // the frame's own permutation: the next list build or upload re-sorts the handle's slots, the per-slot arrays stay
    HIPCHK(hipMemcpyAsync(B.ids.p, ctx->dev(ctx->cur).id, sizeof(int32_t) * (size_t)ctx->n, hipMemcpyDeviceToDevice,
                          ctx->stream));
    ++B.nsamples;
    B.sampled = true;
    API_END
}

// the last frame's per-slot arrays in particle-id order, into the sampler's staging buffers
static void boo_export(md_ctx *ctx, bool want_qlm)
{
    md_ctx::Boo &B = ctx->boo;
    const size_t n = (size_t)ctx->n;
    if (want_qlm) {
        B.io_d.ensure(2 * (size_t)B.nm * n);
        k_boo_export<<<nblocks(ctx->n), MD_BLOCK, 0, ctx->stream>>>((int)n, B.ids.p, (int)n, B.nm, nullptr, nullptr, nullptr, nullptr,
                                                              B.qlm.p, nullptr, nullptr, nullptr, nullptr, B.io_d.p);
    } else {
        B.io_d.ensure(2 * n);
        B.io_i.ensure(2 * n);
        k_boo_export<<<nblocks(ctx->n), MD_BLOCK, 0, ctx->stream>>>((int)n, B.ids.p, (int)n, B.nm, B.nnb.p, B.q.p, B.qbar.p, B.nconn.p,
                                                              nullptr, B.io_i.p, B.io_d.p, B.io_d.p + n, B.io_i.p + n, nullptr);
    }
    HIPCHK(hipGetLastError());
}

int md_boo_particles(md_ctx *ctx, int32_t *nnb, double *q, double *qbar, int32_t *nconn)
{
    API_BEGIN
    md_ctx::Boo &B = sampler_of(ctx, &md_ctx::boo, "md_boo_particles", "boo");
    if (!B.sampled) throw HipError("md_boo_particles: no frame sampled yet (call md_boo_sample first)");
    const size_t n = (size_t)ctx->n;
    boo_export(ctx, false);
    hipStream_t st = ctx->stream;
    if (nnb) HIPCHK(hipMemcpyAsync(nnb, B.io_i.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (nconn) HIPCHK(hipMemcpyAsync(nconn, B.io_i.p + n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (q) HIPCHK(hipMemcpyAsync(q, B.io_d.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (qbar) HIPCHK(hipMemcpyAsync(qbar, B.io_d.p + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

int md_boo_qlm(md_ctx *ctx, double *qlm)
{
    API_BEGIN
    md_ctx::Boo &B = sampler_of(ctx, &md_ctx::boo, "md_boo_qlm", "boo");
    if (!B.sampled) throw HipError("md_boo_qlm: no frame sampled yet (call md_boo_sample first)");
    if (!qlm) throw HipError("md_boo_qlm: qlm is null");
    boo_export(ctx, true);
    HIPCHK(hipMemcpyAsync(qlm, B.io_d.p, sizeof(double) * 2 * (size_t)B.nm * (size_t)ctx->n, hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    API_END
}

int md_boo_read(md_ctx *ctx, int64_t *nsamples, double *sum_fr, int64_t *hist_q, int64_t *hist_qbar, int64_t *hist_nnb,
                int64_t *hist_conn, double *series)
{
    API_BEGIN
    md_ctx::Boo &B = sampler_of(ctx, &md_ctx::boo, "md_boo_read", "boo");
    hipStream_t st = ctx->stream;
    const size_t nb = (size_t)B.nbins, ns = MD_BOO_NCLAMP + 1, w = sizeof(unsigned long long);
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "histogram words are read back as int64_t");
    if (sum_fr) HIPCHK(hipMemcpyAsync(sum_fr, B.sum_fr.p, sizeof(double) * MD_BOO_NFR, hipMemcpyDeviceToHost, st));
    if (hist_q) HIPCHK(hipMemcpyAsync(hist_q, B.hist.p, w * nb, hipMemcpyDeviceToHost, st));
    if (hist_qbar) HIPCHK(hipMemcpyAsync(hist_qbar, B.hist.p + nb, w * nb, hipMemcpyDeviceToHost, st));
    if (hist_nnb) HIPCHK(hipMemcpyAsync(hist_nnb, B.hist.p + 2 * nb, w * ns, hipMemcpyDeviceToHost, st));
    if (hist_conn) HIPCHK(hipMemcpyAsync(hist_conn, B.hist.p + 2 * nb + ns, w * ns, hipMemcpyDeviceToHost, st));
    if (series && B.nseries > 0)
        HIPCHK(hipMemcpyAsync(series, B.series.p, sizeof(double) * MD_BOO_NFR * (size_t)B.nseries, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nsamples) *nsamples = B.nsamples;
    API_END
}

int md_boo_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::boo, "md_boo_reset", "boo");
    boo_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Clusters (md_cluster.hpp): a sample walks the OUTER rows as md_boo_sample does, reads positions, rows and -- SOLID --
// the bond-order sampler's last frame, and writes only the sampler's own buffers.
int md_cluster_setup(md_ctx *ctx, double r_bond, int members, int max_size, int64_t nseries)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_cluster_setup: not available on a slab-decomposition handle");
    if (!(r_bond > 0.0) || !std::isfinite(r_bond)) throw HipError("md_cluster_setup: r_bond must be finite and > 0");
    if (r_bond > ctx->rc) {
        char b[256];
        snprintf(b, sizeof b, "md_cluster_setup: r_bond = %.17g exceeds the list cutoff %.17g (the rows are complete only up to it)",
                 r_bond, ctx->rc);
        throw HipError(b);
    }
    if (members != MD_CLUSTER_ALL && members != MD_CLUSTER_SOLID)
        throw HipError("md_cluster_setup: members must be MD_CLUSTER_ALL or MD_CLUSTER_SOLID");
    check_range("md_cluster_setup", "max_size", max_size, 1, MD_CL_MAX_SIZE);
    if (nseries < 0 || nseries > MD_CL_MAX_SERIES) throw HipError("md_cluster_setup: nseries must be in 0..1048576");
    if (members == MD_CLUSTER_SOLID && !ctx->boo.on)
        throw HipError("md_cluster_setup: MD_CLUSTER_SOLID needs the bond-order sampler (call md_boo_setup first)");
    md_ctx::Cluster &C = ctx->cluster;
    C.on = false;
    C.sampled = false;
    C.members = members;
    C.max_size = max_size;
    C.rb = r_bond;
    C.rb2 = r_bond * r_bond;
    C.nseries = nseries;
    const size_t n = (size_t)ctx->n;
    C.parent.alloc(n);
    C.root.alloc(n);
    C.count.alloc(n);
    C.minid.alloc(n);
    C.ids.alloc(n);
    C.mem.alloc(n);
    C.mask.alloc(members == MD_CLUSTER_SOLID ? n : 1);
    C.part.alloc((size_t)MD_CL_NPART * std::max(nblocks(ctx->n), 1));
    C.deg.alloc((size_t)std::max(nblocks(ctx->n), 1));
    C.hist.alloc((size_t)max_size + 1);
    C.sum_fr.alloc(MD_CL_NFR);
    C.series.alloc((size_t)MD_CL_NFR * std::max<int64_t>(nseries, 1));
    cluster_zero(ctx);
    C.on = true;
    API_END
}

int md_cluster_sample(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_cluster_sample");
    md_ctx::Cluster &C = sampler_of(ctx, &md_ctx::cluster, "md_cluster_sample", "cluster");
    if (C.members == MD_CLUSTER_SOLID && !(ctx->boo.on && ctx->boo.sampled))
        throw HipError("md_cluster_sample: MD_CLUSTER_SOLID needs a bond-order frame (call md_boo_sample first)");
    if (!ctx->list_valid) rebuild(ctx); // the build md_compute_forces / md_run would make at these positions
    if (ctx->dim == 3)
        launch_cluster<3>(ctx);
    else
        launch_cluster<2>(ctx);
    HIPCHK(hipGetLastError());
    // the frame's own permutation: the next list build or upload re-sorts the handle's slots, the per-slot arrays stay
    HIPCHK(hipMemcpyAsync(C.ids.p, ctx->dev(ctx->cur).id, sizeof(int32_t) * (size_t)ctx->n, hipMemcpyDeviceToDevice,
                          ctx->stream));
    ++C.nsamples;
    C.sampled = true;
    API_END
}

int md_cluster_particles(md_ctx *ctx, int32_t *label, int32_t *size)
{
    API_BEGIN
    md_ctx::Cluster &C = sampler_of(ctx, &md_ctx::cluster, "md_cluster_particles", "cluster");
    if (!C.sampled) throw HipError("md_cluster_particles: no frame sampled yet (call md_cluster_sample first)");
    const size_t n = (size_t)ctx->n;
    hipStream_t st = ctx->stream;
    C.io_i.ensure(2 * n);
    k_cl_export<<<nblocks(ctx->n), MD_BLOCK, 0, st>>>((int)n, C.ids.p, C.root.p, C.count.p, C.minid.p, C.io_i.p, C.io_i.p + n);
    HIPCHK(hipGetLastError());
    if (label) HIPCHK(hipMemcpyAsync(label, C.io_i.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (size) HIPCHK(hipMemcpyAsync(size, C.io_i.p + n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

int md_cluster_read(md_ctx *ctx, int64_t *nsamples, int64_t *sum_fr, int64_t *hist_size, int64_t *series)
{
    API_BEGIN
    md_ctx::Cluster &C = sampler_of(ctx, &md_ctx::cluster, "md_cluster_read", "cluster");
    hipStream_t st = ctx->stream;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t) && sizeof(long long) == sizeof(int64_t),
                  "the device words are read back as int64_t");
    if (sum_fr) HIPCHK(hipMemcpyAsync(sum_fr, C.sum_fr.p, sizeof(int64_t) * MD_CL_NFR, hipMemcpyDeviceToHost, st));
    if (hist_size)
        HIPCHK(hipMemcpyAsync(hist_size, C.hist.p, sizeof(int64_t) * ((size_t)C.max_size + 1), hipMemcpyDeviceToHost, st));
    if (series && C.nseries > 0)
        HIPCHK(hipMemcpyAsync(series, C.series.p, sizeof(int64_t) * MD_CL_NFR * (size_t)C.nseries, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nsamples) *nsamples = C.nsamples;
    API_END
}

int md_cluster_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::cluster, "md_cluster_reset", "cluster");
    cluster_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Cage-relative dynamics and bond breaking (md_cage.hpp): an origin store walks the OUTER rows as md_boo_sample does and
// never evaluates the potential -- so it serves every potential, a user's included -- and a sample reads two exported
// frames and the table; both write only the sampler's own buffers.
int md_cage_setup(md_ctx *ctx, int nslots, int nrows, double r_neigh, double r_break, int scaled, int max_neigh,
                  const double *q, int nq)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_cage_setup: not available on a slab-decomposition handle");
    char b[360];
    check_range("md_cage_setup", "nslots", nslots, 1, MD_DYN_MAX_SLOTS);
    check_nrows("md_cage_setup", nrows, 1);
    if (!(r_neigh > 0.0) || !std::isfinite(r_neigh)) throw HipError("md_cage_setup: r_neigh must be finite and > 0");
    if (!std::isfinite(r_break) || !(r_break >= r_neigh)) {
        snprintf(b, sizeof b, "md_cage_setup: r_break must be finite and >= r_neigh = %.17g, got %.17g", r_neigh, r_break);
        throw HipError(b);
    }
    check_range("md_cage_setup", "scaled", scaled, 0, 1);
    check_range("md_cage_setup", "max_neigh", max_neigh, 1, MD_CAGE_MAX_NEIGH);
    check_q("md_cage_setup", q, nq);
    md_ctx::Cage &G = ctx->cage;
    G.on = false;
    G.sampled = false;
    const int64_t n = ctx->n;
    const int d = ctx->dim;
    const size_t entries = (size_t)nslots * (size_t)n * (size_t)max_neigh;
    // MDHIP_CAGE_ALLOC_LIMIT=bytes refuses a table above this size
    snprintf(b, sizeof b, "the neighbour table (nslots*N*max_neigh*(4+8*d) = %d*%lld*%d*(4+8*%d))", nslots, (long long)n,
             max_neigh, d);
    alloc_or_refuse("md_cage_setup", "MDHIP_CAGE_ALLOC_LIMIT", entries * (4 + 8 * (size_t)d), b,
                    std::make_pair(&G.nid, entries), std::make_pair(&G.del, entries * d));
    const size_t frame = (size_t)n * d;
    const int nquant = 2 + nq;
    const int nblk = blocks_of(n, MD_DYN_BLOCK * MD_DYN_PPT);
    G.ox.alloc((size_t)nslots * frame);
    G.oi.alloc((size_t)nslots * frame);
    G.nnb.alloc((size_t)nslots * n);
    G.sig.alloc((size_t)nslots * n);
    G.cx.alloc(frame);
    G.ci.alloc(frame);
    G.part.alloc((size_t)MD_CAGE_MAX_BATCH * nquant * std::max(nblk, 1));
    G.sums.alloc((size_t)nrows * nquant);
    G.counts.alloc((size_t)nrows * MD_CAGE_NCOUNT);
    G.hist.alloc((size_t)nrows * MD_CAGE_NHIST);
    G.overflow.alloc(1);
    G.l_nnb.alloc((size_t)n);
    G.l_broken.alloc((size_t)n);
    G.l_d2.alloc((size_t)n);
    G.sr.init(nslots, nrows);
    G.nq = nq;
    G.max_neigh = max_neigh;
    G.scaled = scaled;
    G.r_neigh = r_neigh;
    G.r_break = r_break;
    G.q.assign(q, q + nq);
    HIPCHK(hipMemsetAsync(G.overflow.p, 0, sizeof(unsigned long long), ctx->stream));
    cage_zero(ctx);
    G.on = true;
    API_END
}

int md_cage_origin(md_ctx *ctx, int slot)
{
    API_BEGIN
    md_ctx::Cage &G = sampler_of(ctx, &md_ctx::cage, "md_cage_origin", "cage");
    require_state(ctx, "md_cage_origin");
    G.sr.check_slot("md_cage_origin", slot);
    const double reach = G.r_neigh * (G.scaled ? ctx->sigma_max : 1.0);
    if (reach > ctx->rc) {
        char b[320];
        snprintf(b, sizeof b,
                 "md_cage_origin: the neighbour radius %.17g (r_neigh%s) exceeds the list cutoff %.17g (the rows are "
                 "complete only up to it)",
                 reach, G.scaled ? " times the largest diameter" : "", ctx->rc);
        throw HipError(b);
    }
    if (!ctx->list_valid) rebuild(ctx); // the build md_compute_forces / md_run would make at these positions
    const size_t frame = (size_t)ctx->n * ctx->dim;
    export_frame(ctx, G.ox.p + (size_t)slot * frame, G.oi.p + (size_t)slot * frame);
    if (ctx->dim == 3)
        launch_cage_origin<3>(ctx, slot);
    else
        launch_cage_origin<2>(ctx, slot);
    HIPCHK(hipGetLastError());
    G.sr.filled[slot] = 1;
    API_END
}

int md_cage_sample(md_ctx *ctx, const int32_t *slots, const int32_t *rows, int count)
{
    API_BEGIN
    md_ctx::Cage &G = sampler_of(ctx, &md_ctx::cage, "md_cage_sample", "cage");
    require_state(ctx, "md_cage_sample");
    G.sr.check_batch("md_cage_sample", slots, rows, count, "store an origin with md_cage_origin first");
    if (count == 0) return 0;
    const size_t n = (size_t)ctx->n;
    G.disp.ensure((size_t)std::min(count, MD_CAGE_MAX_BATCH) * ctx->dim * n);
    export_frame(ctx, G.cx.p, G.ci.p);
    const DynParams P = dyn_params(ctx, &G.q);
    CageSample A{};
    A.max_neigh = G.max_neigh;
    A.scaled = G.scaled;
    A.r_break = G.r_break;
    A.nnb = G.nnb.p;
    A.nid = G.nid.p;
    A.del = G.del.p;
    A.sig = G.sig.p;
    A.disp = G.disp.p;
    A.part = G.part.p;
    A.counts = G.counts.p;
    A.hist = G.hist.p;
    A.o_nnb = G.l_nnb.p;
    A.o_broken = G.l_broken.p;
    A.o_d2 = G.l_d2.p;
    for (int i0 = 0; i0 < count; i0 += MD_CAGE_MAX_BATCH) {
        const DynBatch B = batch_from<DynBatch>(slots, rows, i0, count, MD_CAGE_MAX_BATCH);
        A.keep = (i0 + B.count == count) ? B.count - 1 : -1; // the call's last entry stays readable (md_cage_particles)
        if (ctx->dim == 3)
            launch_cage_sample<3>(ctx, P, B, A);
        else
            launch_cage_sample<2>(ctx, P, B, A);
        HIPCHK(hipGetLastError());
        G.sr.count_rows(B.row, B.count);
    }
    G.sampled = true;
    API_END
}

int md_cage_particles(md_ctx *ctx, int32_t *nnb, double *d2cr, int32_t *broken)
{
    API_BEGIN
    md_ctx::Cage &G = sampler_of(ctx, &md_ctx::cage, "md_cage_particles", "cage");
    if (!G.sampled) throw HipError("md_cage_particles: no sample taken yet (call md_cage_sample first)");
    const size_t n = (size_t)ctx->n;
    hipStream_t st = ctx->stream;
    if (nnb) HIPCHK(hipMemcpyAsync(nnb, G.l_nnb.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (d2cr) HIPCHK(hipMemcpyAsync(d2cr, G.l_d2.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (broken) HIPCHK(hipMemcpyAsync(broken, G.l_broken.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

int md_cage_read(md_ctx *ctx, int64_t *nsamples, double *sums, int64_t *counts, int64_t *hist_broken, int64_t *overflow)
{
    API_BEGIN
    md_ctx::Cage &G = sampler_of(ctx, &md_ctx::cage, "md_cage_read", "cage");
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the device words are read back as int64_t");
    hipStream_t st = ctx->stream;
    const size_t nr = (size_t)G.sr.nrows;
    if (sums) HIPCHK(hipMemcpyAsync(sums, G.sums.p, sizeof(double) * nr * (2 + G.nq), hipMemcpyDeviceToHost, st));
    if (counts) HIPCHK(hipMemcpyAsync(counts, G.counts.p, sizeof(int64_t) * nr * MD_CAGE_NCOUNT, hipMemcpyDeviceToHost, st));
    if (hist_broken)
        HIPCHK(hipMemcpyAsync(hist_broken, G.hist.p, sizeof(int64_t) * nr * MD_CAGE_NHIST, hipMemcpyDeviceToHost, st));
    if (overflow) HIPCHK(hipMemcpyAsync(overflow, G.overflow.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    G.sr.read_counts(nsamples);
    API_END
}

int md_cage_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::cage, "md_cage_reset", "cage");
    cage_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Four-point dynamics (md_chi4.hpp): an origin store and a sample each launch k_export into the sampler's own buffers and
// read nothing else of the state, so the step loop, the list and the cell order are exactly what they would have been
// without them.
int md_chi4_setup(md_ctx *ctx, double a, const int32_t *nvecs, int nvec, int nslots, int nrows)
{
#pragma clang fp contract(off)
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_chi4_setup: not available on a slab-decomposition handle");
    char b[320];
    if (!(a > 0.0) || !std::isfinite(a)) throw HipError("md_chi4_setup: a must be finite and > 0");
    check_range("md_chi4_setup", "nvec", nvec, 0, MD_CHI4_MAX_VEC);
    if (nvec > 0 && !nvecs) throw HipError("md_chi4_setup: n is null");
    check_range("md_chi4_setup", "nslots", nslots, 1, MD_CHI4_MAX_SLOTS);
    check_nrows("md_chi4_setup", nrows, 1);
    const int dim = ctx->dim;
    check_wave_vectors("md_chi4_setup", nvecs, nvec, dim, "W(0) = Q carries no information");
    md_ctx::Chi4 &X = ctx->chi4;
    X.on = false;
    const int64_t n = ctx->n;
    const size_t frame = (size_t)n * dim, slots_size = (size_t)nslots * frame;
    const int per = nvec > 0 ? 20 : 12; // bytes per coordinate: x, n and -- with vectors -- the fractional coordinate
    // MDHIP_CHI4_ALLOC_LIMIT=bytes refuses origin slots above this size
    snprintf(b, sizeof b, "%d origin slots (nslots*N*d*%d = %d*%lld*%d*%d)", nslots, per, nslots, (long long)n, dim, per);
    alloc_or_refuse("md_chi4_setup", "MDHIP_CHI4_ALLOC_LIMIT", slots_size * per, b, std::make_pair(&X.ox, slots_size),
                    std::make_pair(&X.oi, slots_size), std::make_pair(&X.of, nvec > 0 ? slots_size : (size_t)0));
    const int nwords = (int)((n + 63) / 64);
    hipStream_t st = ctx->stream;
    X.init(nvecs, nvec, dim, n, 2, st);
    X.cx.alloc(frame);
    X.ci.alloc(frame);
    X.wlast.alloc((size_t)nvec * 2);
    X.s4.alloc((size_t)nrows * std::max(nvec, 1));
    X.mask.alloc(nwords);
    X.qcur.alloc(1);
    X.qlast.alloc(1);
    X.irow.alloc((size_t)nrows * MD_CHI4_NROW);
    HIPCHK(hipMemsetAsync(X.qcur.p, 0, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(X.qlast.p, 0, sizeof(long long), st));
    X.sr.init(nslots, nrows);
    X.nwords = nwords;
    X.a = a;
    X.a2 = a * a;
    X.sampled = false;
    chi4_zero(ctx); // (waits)
    X.on = true;
    API_END
}

int md_chi4_origin(md_ctx *ctx, int slot)
{
    API_BEGIN
    md_ctx::Chi4 &X = sampler_of(ctx, &md_ctx::chi4, "md_chi4_origin", "chi4");
    require_state(ctx, "md_chi4_origin");
    X.sr.check_slot("md_chi4_origin", slot);
    const size_t frame = (size_t)ctx->n * ctx->dim;
    double *ox = X.ox.p + (size_t)slot * frame;
    export_frame(ctx, ox, X.oi.p + (size_t)slot * frame);
    if (X.nvec > 0) launch_frac(ctx, ox, X.of.p + (size_t)slot * frame);
    X.sr.filled[slot] = 1;
    API_END
}

int md_chi4_sample(md_ctx *ctx, const int32_t *slots, const int32_t *rows, int count)
{
    API_BEGIN
    md_ctx::Chi4 &X = sampler_of(ctx, &md_ctx::chi4, "md_chi4_sample", "chi4");
    require_state(ctx, "md_chi4_sample");
    X.sr.check_batch("md_chi4_sample", slots, rows, count, "store an origin with md_chi4_origin first");
    if (count == 0) return 0;
    // sum_q2 gains at most N^2 per sample: refuse the call before anything is launched if a row could pass the limit
    // (MDHIP_CHI4_SUMQ2_LIMIT=value lowers it from 2^63 - 1: a debug switch, the refusal can be checked at a test size)
    {
        const char *lim = getenv("MDHIP_CHI4_SUMQ2_LIMIT");
        const __int128 limit = lim ? (__int128)strtoull(lim, nullptr, 10) : (__int128)INT64_MAX;
        const __int128 n2 = (__int128)ctx->n * (__int128)ctx->n;
        std::vector<int64_t> ns(X.sr.nsamples);
        for (int i = 0; i < count; ++i) {
            if ((__int128)(ns[rows[i]] + 1) * n2 > limit) {
                char b[240];
                snprintf(b, sizeof b,
                         "md_chi4_sample: row %d already holds %lld samples; one more could overflow sum_q2 ((nsamples + 1) "
                         "N^2 > %s with N = %lld): read and reset first",
                         (int)rows[i], (long long)ns[rows[i]], lim ? lim : "2^63 - 1", (long long)ctx->n);
                throw HipError(b);
            }
            ++ns[rows[i]];
        }
    }
    export_frame(ctx, X.cx.p, X.ci.p);
    const DynParams P = dyn_params(ctx);
    for (int i = 0; i < count; ++i) {
        if (ctx->dim == 3)
            launch_chi4_sample<3>(ctx, P, slots[i], rows[i]);
        else
            launch_chi4_sample<2>(ctx, P, slots[i], rows[i]);
        X.sr.count_rows(rows + i, 1);
        X.sampled = true;
    }
    API_END
}

int md_chi4_last(md_ctx *ctx, int64_t *q, double *w, void *slow_bytes)
{
    uint8_t *slow = static_cast<uint8_t *>(slow_bytes);
    API_BEGIN
    md_ctx::Chi4 &X = sampler_of(ctx, &md_ctx::chi4, "md_chi4_last", "chi4");
    if (!X.sampled) throw HipError("md_chi4_last: no sample taken yet (call md_chi4_sample first)");
    hipStream_t st = ctx->stream;
    long long ql = 0;
    std::vector<unsigned long long> m(slow ? X.nwords : 0);
    if (q) HIPCHK(hipMemcpyAsync(&ql, X.qlast.p, sizeof ql, hipMemcpyDeviceToHost, st));
    if (w && X.nvec) HIPCHK(hipMemcpyAsync(w, X.wlast.p, sizeof(double) * X.nvec * 2, hipMemcpyDeviceToHost, st));
    if (slow) HIPCHK(hipMemcpyAsync(m.data(), X.mask.p, sizeof(unsigned long long) * X.nwords, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (q) *q = ql;
    if (slow)
        for (int64_t i = 0; i < ctx->n; ++i) slow[i] = (uint8_t)((m[i >> 6] >> (i & 63)) & 1ull);
    API_END
}

int md_chi4_read(md_ctx *ctx, int64_t *nsamples, int64_t *sum_q, int64_t *sum_q2, double *s4)
{
    API_BEGIN
    md_ctx::Chi4 &X = sampler_of(ctx, &md_ctx::chi4, "md_chi4_read", "chi4");
    hipStream_t st = ctx->stream;
    std::vector<long long> r((size_t)X.sr.nrows * MD_CHI4_NROW);
    HIPCHK(hipMemcpyAsync(r.data(), X.irow.p, sizeof(long long) * r.size(), hipMemcpyDeviceToHost, st));
    if (s4 && X.nvec) HIPCHK(hipMemcpyAsync(s4, X.s4.p, sizeof(double) * X.sr.nrows * X.nvec, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < X.sr.nrows; ++k) {
        if (sum_q) sum_q[k] = r[(size_t)k * MD_CHI4_NROW];
        if (sum_q2) sum_q2[k] = r[(size_t)k * MD_CHI4_NROW + 1];
        if (nsamples) nsamples[k] = r[(size_t)k * MD_CHI4_NROW + 2];
    }
    API_END
}

int md_chi4_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::chi4, "md_chi4_reset", "chi4");
    chi4_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Currents, C_L / C_T(q, t) and the VACF (md_cur.hpp): a sample launches k_export into the sampler's own frame buffers
// (x and v) and reads nothing else of the state, so the step loop, the list and the cell order are what they would have
// been without it.
int md_cur_setup(md_ctx *ctx, const int32_t *nvecs, const double *e, int nvec, int nslots, int nrows, int vacf)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_cur_setup: not available on a slab-decomposition handle");
    char b[320];
    check_range("md_cur_setup", "vacf", vacf, 0, 1);
    check_range("md_cur_setup", "nvec", nvec, vacf ? 0 : 1, MD_SQ_MAX_VEC);
    if (nvec > 0 && !nvecs) throw HipError("md_cur_setup: n is null");
    if (nvec > 0 && !e) throw HipError("md_cur_setup: e is null");
    check_range("md_cur_setup", "nslots", nslots, 0, MD_SQ_MAX_SLOTS);
    check_nrows("md_cur_setup", nrows, 0);
    const int dim = ctx->dim;
    check_wave_vectors("md_cur_setup", nvecs, nvec, dim, "j(0) = the total momentum, a constant of the motion");
    for (int v = 0; v < nvec; ++v) {
        bool finite = true, zero = true;
        for (int c = 0; c < dim; ++c) {
            finite = finite && std::isfinite(e[(size_t)v * dim + c]);
            zero = zero && e[(size_t)v * dim + c] == 0.0;
        }
        if (!finite || zero) {
            snprintf(b, sizeof b, "md_cur_setup: direction %d must be finite and not all zero", v);
            throw HipError(b);
        }
    }
    md_ctx::Cur &S = ctx->current;
    S.on = false;
    const int64_t n = ctx->n;
    const size_t frame = (size_t)n * dim, slots_size = vacf ? (size_t)nslots * frame : (size_t)0;
    // MDHIP_CUR_ALLOC_LIMIT=bytes refuses velocity origin slots above this size
    snprintf(b, sizeof b, "%d velocity origin slots (nslots*N*d*8 = %d*%lld*%d*8)", nslots, nslots, (long long)n, dim);
    alloc_or_refuse("md_cur_setup", "MDHIP_CUR_ALLOC_LIMIT", slots_size * 8, b, std::make_pair(&S.ov, slots_size));
    const int zblk = blocks_of(n, MD_CUR_VACF_BLOCK * MD_CUR_VACF_PPT);
    const size_t nv = (size_t)nvec;
    hipStream_t st = ctx->stream;
    S.init(nvecs, nvec, dim, n, 2 * dim, st);
    S.e.alloc(nv * dim);
    S.cx.alloc(frame);
    S.cv.alloc(frame);
    S.ci.alloc(frame);
    S.fr.alloc(nvec ? frame : 0);
    S.va.alloc(nvec ? frame : 0);
    S.jl.alloc(nv * 2 * dim);
    S.s_tot.alloc(nv);
    S.s_long.alloc(nv);
    S.c_tot.alloc((size_t)nrows * nv);
    S.c_long.alloc((size_t)nrows * nv);
    S.org.alloc((size_t)nslots * nv * 2 * dim);
    S.zpart.alloc(vacf ? (size_t)MD_CUR_MAX_BATCH * std::max(zblk, 1) : 0);
    S.z.alloc(vacf ? (size_t)nrows + 1 : 0);
    if (nvec) {
        HIPCHK(hipMemcpyAsync(S.e.p, e, sizeof(double) * nv * dim, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(S.jl.p, 0, sizeof(double) * nv * 2 * dim, st));
        if (nslots) HIPCHK(hipMemsetAsync(S.org.p, 0, sizeof(double) * nslots * nv * 2 * dim, st));
    }
    S.vacf = vacf != 0;
    S.sr.init(nslots, nrows);
    S.zblk = zblk;
    S.sampled = false;
    cur_zero(ctx); // (waits: the tables are host memory)
    S.on = true;
    API_END
}

int md_cur_sample(md_ctx *ctx, int add_static, const int32_t *slots, const int32_t *rows, int count, int origin_slot)
{
    API_BEGIN
    md_ctx::Cur &S = sampler_of(ctx, &md_ctx::current, "md_cur_sample", "cur");
    require_state(ctx, "md_cur_sample");
    S.sr.check_batch("md_cur_sample", slots, rows, count, "store an origin with origin_slot first");
    S.sr.check_origin("md_cur_sample", origin_slot);
    hipStream_t st = ctx->stream;
    const int n = (int)ctx->n, dim = ctx->dim;
    export_frame(ctx, S.cx.p, S.ci.p, S.cv.p);
    if (S.nvec > 0) {
        launch_frac(ctx, S.cx.p, S.fr.p);
        if (dim == 3)
            launch_cur_modes<3>(ctx, st);
        else
            launch_cur_modes<2>(ctx, st);
        for_batches<CurBatch>(slots, rows, count, MD_CUR_MAX_BATCH, [&](const CurBatch &B, bool first, bool last) {
            if (dim == 3)
                launch_cur_reduce<3>(ctx, st, first, add_static != 0, B, last ? origin_slot : -1);
            else
                launch_cur_reduce<2>(ctx, st, first, add_static != 0, B, last ? origin_slot : -1);
        });
    }
    if (S.vacf) {
        // the equal-time pair (the frame against itself, into the row after the lag rows) first, then the call's pairs
        std::vector<int32_t> zs, zr;
        if (add_static) {
            zs.push_back(-1);
            zr.push_back(S.sr.nrows);
        }
        zs.insert(zs.end(), slots, slots + count);
        zr.insert(zr.end(), rows, rows + count);
        const int zcount = (int)zs.size();
        for (int i0 = 0; i0 < zcount; i0 += MD_CUR_MAX_BATCH) {
            const CurBatch B = batch_from<CurBatch>(zs.data(), zr.data(), i0, zcount, MD_CUR_MAX_BATCH);
            const dim3 grid(S.zblk, B.count);
            if (dim == 3)
                k_cur_vacf<3><<<grid, MD_CUR_VACF_BLOCK, 0, st>>>(n, S.zblk, B, S.cv.p, S.ov.p, S.zpart.p);
            else
                k_cur_vacf<2><<<grid, MD_CUR_VACF_BLOCK, 0, st>>>(n, S.zblk, B, S.cv.p, S.ov.p, S.zpart.p);
            HIPCHK(hipGetLastError());
            if (dim == 3)
                k_cur_vacf_reduce<3><<<1, MD_CUR_VACF_REDUCE_BLOCK, 0, st>>>(S.zblk, B, S.zpart.p, S.z.p);
            else
                k_cur_vacf_reduce<2><<<1, MD_CUR_VACF_REDUCE_BLOCK, 0, st>>>(S.zblk, B, S.zpart.p, S.z.p);
            HIPCHK(hipGetLastError());
        }
        if (origin_slot >= 0) {
            const size_t frame = (size_t)n * dim;
            HIPCHK(hipMemcpyAsync(S.ov.p + (size_t)origin_slot * frame, S.cv.p, sizeof(double) * frame,
                                  hipMemcpyDeviceToDevice, st));
        }
    }
    S.sampled = true;
    if (add_static) ++S.nstatic;
    S.sr.count_rows(rows, count);
    if (origin_slot >= 0) S.sr.filled[origin_slot] = 1;
    API_END
}

int md_cur_last(md_ctx *ctx, double *j)
{
    API_BEGIN
    md_ctx::Cur &S = sampler_of(ctx, &md_ctx::current, "md_cur_last", "cur");
    if (!S.sampled) throw HipError("md_cur_last: no frame has been sampled since md_cur_setup");
    if (!j) throw HipError("md_cur_last: j is null");
    if (S.nvec)
        HIPCHK(hipMemcpyAsync(j, S.jl.p, sizeof(double) * S.nvec * 2 * ctx->dim, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    API_END
}

int md_cur_read(md_ctx *ctx, int64_t *nstatic, double *s_tot, double *s_long, int64_t *nsamples, double *c_tot,
                double *c_long, double *z)
{
    API_BEGIN
    md_ctx::Cur &S = sampler_of(ctx, &md_ctx::current, "md_cur_read", "cur");
    if (z && !S.vacf) throw HipError("md_cur_read: z needs a setup with vacf != 0");
    hipStream_t st = ctx->stream;
    const size_t nv = (size_t)S.nvec, nc = (size_t)S.sr.nrows * nv;
    if (s_tot && nv) HIPCHK(hipMemcpyAsync(s_tot, S.s_tot.p, sizeof(double) * nv, hipMemcpyDeviceToHost, st));
    if (s_long && nv) HIPCHK(hipMemcpyAsync(s_long, S.s_long.p, sizeof(double) * nv, hipMemcpyDeviceToHost, st));
    if (c_tot && nc) HIPCHK(hipMemcpyAsync(c_tot, S.c_tot.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
    if (c_long && nc) HIPCHK(hipMemcpyAsync(c_long, S.c_long.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
    if (z) HIPCHK(hipMemcpyAsync(z, S.z.p, sizeof(double) * ((size_t)S.sr.nrows + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nstatic) *nstatic = S.nstatic;
    S.sr.read_counts(nsamples);
    API_END
}

int md_cur_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::current, "md_cur_reset", "cur");
    cur_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Marked pair correlations (md_mpc.hpp): md_rdf_sample's pipeline on buffers of its own with a mark carried along; a
// sample reads the state, the marks and -- MD_MPC_BOO -- the bond-order sampler's last frame, and writes only the
// sampler's own buffers.
int md_mpc_setup(md_ctx *ctx, int source, double r_max, int nbins, int nc, const double *weights, double tmax)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_mpc_setup: not available on a slab-decomposition handle");
    if (source != MD_MPC_BOO && source != MD_MPC_USER) throw HipError("md_mpc_setup: source must be MD_MPC_BOO or MD_MPC_USER");
    if (!(r_max > 0.0) || !std::isfinite(r_max)) throw HipError("md_mpc_setup: r_max must be finite and > 0");
    check_range("md_mpc_setup", "nbins", nbins, 1, MD_MPC_MAX_BINS);
    MpcWeights W{};
    if (source == MD_MPC_BOO) {
        const md_ctx::Boo &B = ctx->boo;
        if (!B.on) throw HipError("md_mpc_setup: MD_MPC_BOO needs the bond-order sampler (call md_boo_setup first)");
        // t_ij = pref (Re q_0 q_0' + Im q_0 q_0' + 2 sum_{m>0} ...) <= q_l(i) q_l(j) <= 1
        nc = 2 * B.nm;
        for (int c = 0; c < nc; ++c) W.w[c] = B.coef.pref * (c < 2 ? 1.0 : 2.0);
        tmax = 1.0;
    } else {
        check_range("md_mpc_setup", "nc", nc, 1, 3);
        if (!weights) throw HipError("md_mpc_setup: weights is null");
        for (int c = 0; c < nc; ++c) {
            if (!std::isfinite(weights[c])) throw HipError("md_mpc_setup: every weight must be finite");
            W.w[c] = weights[c];
        }
        if (!(tmax > 0.0) || !std::isfinite(tmax)) throw HipError("md_mpc_setup: tmax must be finite and > 0");
        // rounded up to a power of two: the scaling by 2^31 / tmax is then exact
        int ex = 0;
        const double mant = std::frexp(tmax, &ex); // tmax = mant 2^ex, mant in [0.5, 1)
        if (mant != 0.5) tmax = std::ldexp(1.0, ex);
        if (ex < -900 || ex > 900) throw HipError("md_mpc_setup: tmax must be in 2^-900..2^900");
    }
    W.scale = 2147483648.0 / tmax;
    W.lim = tmax * (1.0 + 1.0 / 1024.0);
    const RdfGrid grid = pair_walk_grid(ctx, "md_mpc_setup", r_max);
    md_ctx::Mpc &M = ctx->mpc;
    M.on = false;
    M.have_marks = false;
    M.source = source;
    M.nc = nc;
    M.nbins = nbins;
    M.r_max = r_max;
    M.tmax = tmax;
    M.w = W;
    M.grid = grid;
    const size_t lds = mpc_lds_bytes(nbins, nc);
    mpc_dispatch(ctx->dim, nc, [&](auto k) { mpc_set_lds<2, decltype(k)::value>(lds); },
                 [&](auto k) { mpc_set_lds<3, decltype(k)::value>(lds); });
    const size_t n = (size_t)ctx->n;
    const std::vector<double> e2 = squared_edges(r_max, nbins);
    hipStream_t st = ctx->stream;
    M.e2.alloc(nbins + 1);
    M.marks.alloc(source == MD_MPC_USER ? n * nc : 1);
    M.smarks.alloc(n * nc);
    M.inv.alloc(source == MD_MPC_BOO ? n : 1);
    M.wrec.alloc(n);
    M.srec.alloc(n);
    M.keys_in.alloc(n);
    M.keys_out.alloc(n);
    M.vals_in.alloc(n);
    M.vals_out.alloc(n);
    M.cell_start.alloc((size_t)grid.ncell + 1);
    M.cell_end.alloc((size_t)grid.ncell + 1);
    M.work.alloc(1);
    M.range_error.alloc(1);
    M.cur_cnt.alloc(nbins);
    M.last_cnt.alloc(nbins);
    M.acc_cnt.alloc(nbins);
    M.cur_sum.alloc(nbins);
    M.last_sum.alloc(nbins);
    M.self.alloc(2);
    M.acc_sum.alloc(nbins);
    M.acc_self.alloc(1);
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, M.keys_in.p, M.keys_out.p, M.vals_in.p, M.vals_out.p, n, 0u,
                                     (unsigned)std::max(1, ceil_log2((uint64_t)grid.ncell)), st));
    M.sort_tmp.alloc(tmp_bytes);
    HIPCHK(hipMemcpyAsync(M.e2.p, e2.data(), sizeof(double) * (nbins + 1), hipMemcpyHostToDevice, st));
    mpc_zero(ctx); // (waits: the edge table is a host vector)
    M.on = true;
    API_END
}

int md_mpc_marks(md_ctx *ctx, const double *marks)
{
    API_BEGIN
    md_ctx::Mpc &M = sampler_of(ctx, &md_ctx::mpc, "md_mpc_marks", "mpc");
    if (M.source != MD_MPC_USER) throw HipError("md_mpc_marks: the marks of an MD_MPC_BOO setup are the bond-order frame's");
    if (!marks) throw HipError("md_mpc_marks: marks is null");
    const size_t count = (size_t)ctx->n * M.nc;
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(marks[i])) throw HipError("md_mpc_marks: every mark must be finite");
    HIPCHK(hipMemcpyAsync(M.marks.p, marks, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream)); // (the caller's array)
    M.have_marks = true;
    API_END
}

int md_mpc_sample(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_mpc_sample");
    md_ctx::Mpc &M = sampler_of(ctx, &md_ctx::mpc, "md_mpc_sample", "mpc");
    const md_ctx::Boo &B = ctx->boo;
    const bool boo = M.source == MD_MPC_BOO;
    if (boo) {
        if (!(B.on && B.sampled)) throw HipError("md_mpc_sample: MD_MPC_BOO needs a bond-order frame (call md_boo_sample first)");
        if (2 * B.nm != M.nc)
            throw HipError("md_mpc_sample: the bond-order setup changed since md_mpc_setup (call md_mpc_setup again)");
    } else if (!M.have_marks) {
        throw HipError("md_mpc_sample: no marks yet (call md_mpc_marks first)");
    }
    const int n = (int)ctx->n;
    const RdfGrid &g = M.grid;
    hipStream_t st = ctx->stream;
    DevState s = ctx->dev(ctx->cur);
    if (ctx->dim == 3)
        k_rdf_key<3><<<nblocks(n), MD_BLOCK, 0, st>>>(n, s, ctx->grid, g, M.wrec.p, M.keys_in.p, M.vals_in.p);
    else
        k_rdf_key<2><<<nblocks(n), MD_BLOCK, 0, st>>>(n, s, ctx->grid, g, M.wrec.p, M.keys_in.p, M.vals_in.p);
    HIPCHK(hipGetLastError());
    size_t tmp_bytes = M.sort_tmp.n;
    HIPCHK(rocprim::radix_sort_pairs(M.sort_tmp.p, tmp_bytes, M.keys_in.p, M.keys_out.p, M.vals_in.p, M.vals_out.p,
                                     (size_t)n, 0u, (unsigned)std::max(1, ceil_log2((uint64_t)g.ncell)), st));
    HIPCHK(hipMemsetAsync(M.cell_start.p, 0, sizeof(int32_t) * (g.ncell + 1), st));
    HIPCHK(hipMemsetAsync(M.cell_end.p, 0, sizeof(int32_t) * (g.ncell + 1), st));
    HIPCHK(hipMemsetAsync(M.work.p, 0, sizeof(int32_t), st));
    if (boo) {
        // marks travel by particle id: whatever re-sorted the handle's slots since md_boo_sample does not matter
        k_mpc_inv<<<nblocks(n), MD_BLOCK, 0, st>>>(n, B.ids.p, M.inv.p);
        HIPCHK(hipGetLastError());
    }
    const double *src = boo ? B.qlm.p : M.marks.p;
    const int32_t *inv = boo ? M.inv.p : nullptr;
    const size_t stride_i = boo ? 1 : (size_t)M.nc, stride_c = boo ? (size_t)n : 1;
    const size_t lds = mpc_lds_bytes(M.nbins, M.nc);
    mpc_dispatch(ctx->dim, M.nc,
                 [&](auto k) { mpc_launch<2, decltype(k)::value>(ctx, src, inv, stride_i, stride_c, lds); },
                 [&](auto k) { mpc_launch<3, decltype(k)::value>(ctx, src, inv, stride_i, stride_c, lds); });
    k_mpc_finish<<<nblocks(M.nbins), MD_BLOCK, 0, st>>>(M.nbins, M.cur_cnt.p, M.cur_sum.p, M.self.p, M.last_cnt.p,
                                                        M.last_sum.p, M.self.p + 1, M.acc_cnt.p, M.acc_sum.p,
                                                        M.acc_self.p, M.range_error.p);
    HIPCHK(hipGetLastError());
    ++M.nsamples;
    M.sampled = true;
    API_END
}

int md_mpc_last(md_ctx *ctx, int64_t *cnt, int64_t *sum, int64_t *self)
{
    API_BEGIN
    md_ctx::Mpc &M = sampler_of(ctx, &md_ctx::mpc, "md_mpc_last", "mpc");
    if (!M.sampled) throw HipError("md_mpc_last: no sample yet (call md_mpc_sample first)");
    static_assert(sizeof(unsigned long long) == sizeof(int64_t) && sizeof(long long) == sizeof(int64_t),
                  "the device words are read back as int64_t");
    hipStream_t st = ctx->stream;
    if (cnt) HIPCHK(hipMemcpyAsync(cnt, M.last_cnt.p, sizeof(int64_t) * M.nbins, hipMemcpyDeviceToHost, st));
    if (sum) HIPCHK(hipMemcpyAsync(sum, M.last_sum.p, sizeof(int64_t) * M.nbins, hipMemcpyDeviceToHost, st));
    if (self) HIPCHK(hipMemcpyAsync(self, M.self.p + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

int md_mpc_read(md_ctx *ctx, int64_t *nsamples, int64_t *acc_cnt, double *acc_sum, double *acc_self, double *tmax,
                int32_t *range_error)
{
    API_BEGIN
    md_ctx::Mpc &M = sampler_of(ctx, &md_ctx::mpc, "md_mpc_read", "mpc");
    hipStream_t st = ctx->stream;
    if (acc_cnt) HIPCHK(hipMemcpyAsync(acc_cnt, M.acc_cnt.p, sizeof(int64_t) * M.nbins, hipMemcpyDeviceToHost, st));
    if (acc_sum) HIPCHK(hipMemcpyAsync(acc_sum, M.acc_sum.p, sizeof(double) * M.nbins, hipMemcpyDeviceToHost, st));
    if (acc_self) HIPCHK(hipMemcpyAsync(acc_self, M.acc_self.p, sizeof(double), hipMemcpyDeviceToHost, st));
    if (range_error) HIPCHK(hipMemcpyAsync(range_error, M.range_error.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nsamples) *nsamples = M.nsamples;
    if (tmax) *tmax = M.tmax;
    API_END
}

int md_mpc_reset(md_ctx *ctx)
{
    API_BEGIN
    sampler_of(ctx, &md_ctx::mpc, "md_mpc_reset", "mpc");
    mpc_zero(ctx);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Swap Monte Carlo (md_swap.hpp)
// ---------------------------------------------------------------------------------------------
int md_swap_setup(md_ctx *ctx, double fraction, double max_diameter_difference, uint64_t seed)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_swap_setup: not available on a slab-decomposition handle");
    if (!(fraction > 0.0) || !(fraction <= 1.0)) {
        char b[160];
        snprintf(b, sizeof b, "md_swap_setup: fraction must be in (0, 1], got %.17g", fraction);
        throw HipError(b);
    }
    if (std::isnan(max_diameter_difference)) throw HipError("md_swap_setup: max_diameter_difference is NaN (<= 0 means none)");
    md_ctx::Swap &S = ctx->swap;
    S.on = false;
    S.ran = false;
    S.fraction = fraction;
    S.max_diff = max_diameter_difference > 0.0 ? max_diameter_difference : 0.0;
    S.seed = seed;
    // thr = min(2^32 - 1, floor(fraction 2^32)): fraction 2^32 is exact in a double
    const double t = std::floor(fraction * 4294967296.0);
    S.thr = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
    const size_t n = (size_t)ctx->n;
    S.claim.alloc(n);
    S.livekey.alloc(n);
    S.counts.alloc(MD_SWAP_NCOUNT);
    S.partner.alloc(n);
    S.status.alloc(n);
    S.entry.alloc(n);
    S.members.alloc(2 * n + 4);
    S.blocked.alloc(n + 2);
    S.nmember.alloc(1);
    S.inv.alloc(n);
    S.half.alloc(n + 2);
    S.du.alloc(n);
    S.part.alloc((size_t)std::max(nblocks(ctx->n), 1));
    S.du_acc.alloc(1);
    S.on = true;
    API_END
}

int md_swap_rounds(md_ctx *ctx, int64_t nrounds, double ktemp, int64_t first_round, int64_t *counts, int64_t *decided,
                   double *du_accepted, double *energy, double *virial)
{
    API_BEGIN
    require_state(ctx, "md_swap_rounds");
    md_ctx::Swap &S = sampler_of(ctx, &md_ctx::swap, "md_swap_rounds", "swap");
    if (!(ktemp > 0.0) || !std::isfinite(ktemp)) throw HipError("md_swap_rounds: ktemp must be finite and > 0");
    if (nrounds < 0 || nrounds > 0x3fffffff) throw HipError("md_swap_rounds: nrounds must be in 0..2^30");
    if (first_round < 0) throw HipError("md_swap_rounds: first_round must be >= 0");
    if (ctx->pot_kind == POT_CUSTOM)
        throw HipError("md_swap_rounds: not available for a run-time compiled potential (its pair energy is not reachable "
                       "from the swap kernel)");
    if (ctx->uniform_sigma) throw HipError("md_swap_rounds: all diameters are equal: there is nothing to exchange");
    ctx->hess.frozen = false; // (diameters are about to change)
    if (!ctx->list_valid) rebuild(ctx); // the build md_compute_forces / md_run would make at these positions
    hipStream_t st = ctx->stream;
    const int n = (int)ctx->n;
    const int nb = ctx->nblk;
    DevState s = ctx->dev(ctx->cur);
    SwapBufs B{};
    B.n = n;
    B.claim = S.claim.p;
    B.livekey = S.livekey.p;
    B.partner = S.partner.p;
    B.status = S.status.p;
    B.entry = S.entry.p;
    B.members = S.members.p;
    B.half = S.half.p;
    B.blocked = S.blocked.p;
    B.nmember = S.nmember.p;
    B.du = S.du.p;
    B.inv = S.inv.p;
    B.counts = S.counts.p;
    B.partials = S.part.p;
    B.du_acc = S.du_acc.p;
    SwapRows V{};
    V.n = n;
    V.nghost = (int)ctx->nghost;
    V.cap = (long long)ctx->cap;
    V.id = s.id;
    V.maxn = ctx->maxn;
    V.rowlen = ctx->nmax_tile.p;
    V.gowner = ctx->gowner.p;
    if (ctx->use_tiles) {
        V.rows16 = ctx->nlist16.p;
        V.rs = ctx->tile_rs;
        V.halo = ctx->halo.p;
        V.hcap = ctx->hcap;
        V.halo_count = ctx->halo_count.p;
    } else {
        if (!ctx->have_nlist32) throw HipError("internal: neither tiled nor 32-bit rows exist");
        V.rows32 = ctx->nlist.p;
    }
    HIPCHK(hipMemsetAsync(S.claim.p, 0xff, sizeof(unsigned long long) * (size_t)n, st));
    HIPCHK(hipMemsetAsync(S.livekey.p, 0xff, sizeof(unsigned long long) * (size_t)n, st));
    HIPCHK(hipMemsetAsync(S.counts.p, 0, sizeof(unsigned long long) * MD_SWAP_NCOUNT, st));
    HIPCHK(hipMemsetAsync(S.nmember.p, 0, sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(S.du_acc.p, 0, sizeof(double), st));
    k_swap_inv<<<nb, MD_BLOCK, 0, st>>>(n, s.id, S.inv.p);
    // one wave per member, at most n members: never more blocks than that needs
    const int grid = (int)std::min<int64_t>(MD_SWAP_WALK_BLOCKS, std::max<int64_t>(1, ((int64_t)n + 3) / 4));
    for (int64_t r = 0; r < nrounds; ++r) {
        const long long round = (long long)(first_round + r);
        k_swap_propose<<<nb, MD_BLOCK, 0, st>>>(B, (unsigned long long)S.seed, round, S.thr);
        k_swap_live<<<nb, MD_BLOCK, 0, st>>>(B, (unsigned long long)S.seed, round);
        if (ctx->dim == 3)
            launch_swap_walk<3>(ctx, V, s, B, grid);
        else
            launch_swap_walk<2>(ctx, V, s, B, grid);
        k_swap_decide<<<nb, MD_BLOCK, 0, st>>>(B, s, (unsigned long long)S.seed, round, ktemp, S.max_diff);
        k_swap_finish<<<1, 1024, 0, st>>>(nb, B);
    }
    HIPCHK(hipGetLastError());
    if (nrounds > 0) S.ran = true;
    // Every copy of a diameter the handle holds: the real ghost records are copies of their
    // owners' whole records; the other position buffer becomes a copy of this one; the step records are rebuilt from
    // pos[] by every step loop's entry.  The rows do not depend on the diameters and stay as they are.
    launch_ghost_update(ctx, -1);
    HIPCHK(hipMemcpyAsync(ctx->sb[ctx->cur ^ 1].pos.p, ctx->sb[ctx->cur].pos.p, sizeof(double4) * (size_t)ctx->next,
                          hipMemcpyDeviceToDevice, st));
    // forces, U and W of the new diameters (velocity-Verlet's next half-kick reads the forces)
    launch_force(ctx, true, false, 0.0, -1, 1);
    launch_finalize(ctx, true, false, 1.0, 0.0, -1);
    HIPCHK(hipGetLastError());
    unsigned long long hc[MD_SWAP_NCOUNT];
    double hdu = 0.0;
    HIPCHK(hipMemcpyAsync(hc, S.counts.p, sizeof hc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hdu, S.du_acc.p, sizeof hdu, hipMemcpyDeviceToHost, st));
    Scalars h = read_scalars(ctx); // (the call's one wait)
    if (counts) {
        counts[0] = 0;
        for (int c = MD_SWAP_VOID; c <= MD_SWAP_ACCEPTED; ++c) counts[0] += (int64_t)hc[c];
        counts[1] = (int64_t)hc[MD_SWAP_VOID];
        counts[2] = (int64_t)hc[MD_SWAP_LOST];
        counts[3] = (int64_t)hc[MD_SWAP_BLOCKED];
        counts[4] = (int64_t)hc[MD_SWAP_FILTERED];
        counts[5] = (int64_t)hc[MD_SWAP_ACCEPTED];
    }
    if (decided) *decided = (int64_t)(hc[MD_SWAP_REJECTED] + hc[MD_SWAP_ACCEPTED]);
    if (du_accepted) *du_accepted = hdu;
    if (energy) *energy = h.U;
    if (virial) *virial = h.W;
    API_END
}

int md_swap_last(md_ctx *ctx, int32_t *partner, int32_t *status, double *du)
{
    API_BEGIN
    md_ctx::Swap &S = sampler_of(ctx, &md_ctx::swap, "md_swap_last", "swap");
    if (!S.ran) throw HipError("md_swap_last: no round has run yet (call md_swap_rounds first)");
    const size_t n = (size_t)ctx->n;
    hipStream_t st = ctx->stream;
    if (partner) HIPCHK(hipMemcpyAsync(partner, S.partner.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (status) HIPCHK(hipMemcpyAsync(status, S.status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (du) HIPCHK(hipMemcpyAsync(du, S.du.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

int md_diameters(md_ctx *ctx, double *diameters)
{
    API_BEGIN
    require_state(ctx, "md_diameters");
    if (ctx->dom.on) throw HipError("md_diameters: not available on a slab-decomposition handle");
    if (!diameters) throw HipError("md_diameters: diameters is null");
    ctx->io_d.ensure((size_t)ctx->n);
    k_swap_diameters<<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, ctx->dev(ctx->cur), ctx->io_d.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(diameters, ctx->io_d.p, sizeof(double) * (size_t)ctx->n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    API_END
}

// ---------------------------------------------------------------------------------------------
// Hessian of the pair energy (md_hess.hpp): walks the OUTER rows as md_stress_sample does, reads
// positions and diameters and writes only its own buffers.
int md_hess_setup(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_hess_setup");
    if (ctx->dom.on) throw HipError("md_hess_setup: not available on a slab-decomposition handle");
    if (ctx->pot_kind == POT_CUSTOM) throw HipError("md_hess_setup: not available with a user potential (MD_POT_CUSTOM)");
    if (!ctx->list_valid) rebuild(ctx); // the build md_compute_forces / md_run would make at these positions
    ctx->hess.ksteps = 0;
    ctx->hess.frozen = true;
    ctx->hess.epoch++;
    API_END
}

int md_hess_apply(md_ctx *ctx, int m, const double *X, double *Y)
{
    API_BEGIN
    md_ctx::Hess &H = hess_of(ctx, "md_hess_apply");
    check_range("md_hess_apply", "m", m, 1, MD_HESS_MAX_M);
    if (!X || !Y) throw HipError("md_hess_apply: X / Y is null");
    const int n = (int)ctx->n, D = ctx->dim, M = hess_block(m);
    const size_t nd = (size_t)n * D;
    hipStream_t st = ctx->stream;
    H.host_io.ensure(nd * m);
    H.xs.ensure(nd * M);
    H.ys.ensure(nd * M);
    const int32_t *id = ctx->dev(ctx->cur).id;
    HIPCHK(hipMemcpyAsync(H.host_io.p, X, sizeof(double) * nd * m, hipMemcpyHostToDevice, st));
    k_hess_import<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, id, D, m, M, H.host_io.p, H.xs.p);
    launch_hess_apply(ctx, M, H.xs.p, H.ys.p);
    k_hess_export<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, id, D, m, M, H.ys.p, H.host_io.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(Y, H.host_io.p, sizeof(double) * nd * m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

int md_hess_blocks(md_ctx *ctx, double *diag)
{
    API_BEGIN
    md_ctx::Hess &H = hess_of(ctx, "md_hess_blocks");
    if (!diag) throw HipError("md_hess_blocks: diag is null");
    const int n = (int)ctx->n, D = ctx->dim;
    const size_t nb = (size_t)n * D * D;
    hipStream_t st = ctx->stream;
    H.diag.ensure(nb);
    H.host_io.ensure(nb);
    launch_hess_diag(ctx, H.diag.p);
    k_hess_export<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, ctx->dev(ctx->cur).id, D * D, 1, 1, H.diag.p, H.host_io.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(diag, H.host_io.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

int md_hess_lanczos(md_ctx *ctx, int ksteps, uint64_t seed, double *alpha, double *beta)
{
    API_BEGIN
    md_ctx::Hess &H = hess_of(ctx, "md_hess_lanczos");
    const int n = (int)ctx->n, D = ctx->dim;
    const size_t nd = (size_t)n * D;
    if (nd <= (size_t)D) throw HipError("md_hess_lanczos: no degrees of freedom besides the translations");
    check_range("md_hess_lanczos", "ksteps", ksteps, 1, (int)std::min<size_t>(nd - D, 1 << 20));
    if (!alpha || !beta) throw HipError("md_hess_lanczos: alpha / beta is null");
    H.ksteps = 0;
    if (ksteps > H.kcap) {
        H.kcap = 0;
        const size_t bytes = sizeof(double) * nd * (size_t)ksteps;
        char what[160];
        snprintf(what, sizeof what, "a Lanczos basis of %d vectors of %zu doubles", ksteps, nd);
        alloc_or_refuse("md_hess_lanczos", "MDHIP_HESS_LIMIT", bytes, what, std::make_pair(&H.basis, nd * (size_t)ksteps));
        H.kcap = ksteps;
    }
    const int nchunk = (int)((nd + MD_HESS_CHUNK - 1) / MD_HESS_CHUNK);
    H.w.ensure(nd);
    H.part.ensure((size_t)(D + ksteps) * nchunk);
    H.coef.ensure((size_t)D + ksteps + 1);
    H.alpha.ensure(ksteps);
    H.beta.ensure(ksteps);
    hipStream_t st = ctx->stream;
    double *V = H.basis.p;
    double *scratch = H.coef.p + D + ksteps; // |start vector|
    k_hess_start<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, ctx->dev(ctx->cur).id, D, (unsigned long long)seed, H.w.p);
    hess_gs_pass(ctx, 0, 0, nullptr);
    hess_gs_pass(ctx, 0, 0, nullptr);
    hess_normalise(ctx, scratch, V);
    for (int j = 0; j < ksteps; ++j) { // no host wait in here
        launch_hess_apply(ctx, 1, V + (size_t)j * nd, H.w.p);
        hess_gs_pass(ctx, j + 1, 1, H.alpha.p + j);
        hess_gs_pass(ctx, j + 1, 2, H.alpha.p + j);
        hess_normalise(ctx, H.beta.p + j, j + 1 < ksteps ? V + (size_t)(j + 1) * nd : nullptr);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(alpha, H.alpha.p, sizeof(double) * ksteps, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(beta, H.beta.p, sizeof(double) * ksteps, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int j = 0; j < ksteps; ++j)
        if (!std::isfinite(alpha[j]) || !std::isfinite(beta[j]) || (j + 1 < ksteps && !(beta[j] > 0.0))) {
            char b[200];
            snprintf(b, sizeof b, "md_hess_lanczos: the iteration broke down at step %d (alpha = %g, beta = %g): an invariant "
                                  "subspace was exhausted; use fewer steps or another seed", j, alpha[j], beta[j]);
            throw HipError(b);
        }
    H.ksteps = ksteps;
    API_END
}

int md_hess_ritz(md_ctx *ctx, int ksteps, int nvec, const double *S, const double *theta, double *modes, double *resid)
{
    API_BEGIN
    md_ctx::Hess &H = hess_of(ctx, "md_hess_ritz");
    if (H.ksteps <= 0) throw HipError("md_hess_ritz: no Lanczos basis for this frame (call md_hess_lanczos first)");
    if (ksteps != H.ksteps) {
        char b[160];
        snprintf(b, sizeof b, "md_hess_ritz: ksteps = %d, but the basis on the device holds %d vectors", ksteps, H.ksteps);
        throw HipError(b);
    }
    check_range("md_hess_ritz", "nvec", nvec, 1, ksteps);
    if (!S || !theta || !modes || !resid) throw HipError("md_hess_ritz: S / theta / modes / resid is null");
    const int n = (int)ctx->n, D = ctx->dim;
    const size_t nd = (size_t)n * D;
    hipStream_t st = ctx->stream;
    const int32_t *id = ctx->dev(ctx->cur).id;
    H.S.ensure((size_t)ksteps * nvec);
    H.xs.ensure(nd * MD_HESS_MAX_M);
    H.ys.ensure(nd * MD_HESS_MAX_M);
    H.host_io.ensure(nd * MD_HESS_MAX_M);
    HIPCHK(hipMemcpyAsync(H.S.p, S, sizeof(double) * (size_t)ksteps * nvec, hipMemcpyHostToDevice, st));
    std::vector<double> hy(nd * MD_HESS_MAX_M);
    for (int c0 = 0; c0 < nvec; c0 += MD_HESS_MAX_M) {
        const int m = std::min(MD_HESS_MAX_M, nvec - c0), M = hess_block(m);
        k_hess_combine<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, D, nd, ksteps, nvec, c0, M, H.basis.p, H.S.p, H.xs.p);
        launch_hess_apply(ctx, M, H.xs.p, H.ys.p);
        k_hess_export<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, id, D, m, M, H.xs.p, H.host_io.p);
        HIPCHK(hipMemcpyAsync(modes + (size_t)c0 * nd, H.host_io.p, sizeof(double) * nd * m, hipMemcpyDeviceToHost, st));
        k_hess_export<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, id, D, m, M, H.ys.p, H.host_io.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hy.data(), H.host_io.p, sizeof(double) * nd * m, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int c = 0; c < m; ++c) { // |H y - theta y|, elements in particle-id order
            const double *y = modes + (size_t)(c0 + c) * nd, *h = hy.data() + (size_t)c * nd;
            double a = 0.0;
            for (size_t e = 0; e < nd; ++e) {
                double r = h[e] - theta[c0 + c] * y[e];
                a += r * r;
            }
            resid[c0 + c] = std::sqrt(a);
        }
    }
    API_END
}

// ---------------------------------------------------------------------------------------------
// Elastic moduli of the frame md_hess_setup froze (md_elas.hpp): reads positions, diameters and the
// OUTER rows, writes only its own buffers.
int md_elas_affine(md_ctx *ctx, double *stress, double *born, double *xi)
{
    API_BEGIN
    md_ctx::Elas &E = elas_of(ctx, "md_elas_affine", false);
    if (!stress || !born) throw HipError("md_elas_affine: stress / born is null");
    const int n = (int)ctx->n, D = ctx->dim;
    const int nc = D == 3 ? 6 : 3, nb = D == 3 ? 15 : 5, nq = nc + nb + 1, M = hess_block(nc);
    hipStream_t st = ctx->stream;
    E.epoch = 0;
    E.xi.ensure((size_t)n * M * D);
    E.bonded.ensure(n);
    E.part.ensure((size_t)nq * ctx->nblk);
    E.sums.ensure(MD_ELAS_MAX_NQ);
    launch_elas_affine(ctx);
    k_elas_affine_finish<<<nq, MD_BLOCK, 0, st>>>(ctx->nblk, nq, E.part.p, 1.0 / ctx->volume, E.sums.p);
    HIPCHK(hipGetLastError());
    double hsum[MD_ELAS_MAX_NQ];
    HIPCHK(hipMemcpyAsync(hsum, E.sums.p, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
    if (xi) {
        E.host_io.ensure((size_t)n * nc * D);
        k_hess_export<<<ctx->nblk, MD_BLOCK, 0, st>>>(n, ctx->dev(ctx->cur).id, D, nc, M, E.xi.p, E.host_io.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(xi, E.host_io.p, sizeof(double) * (size_t)n * nc * D, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < nc; ++s) stress[s] = hsum[s];
    for (int s = 0; s < nc; ++s)
        for (int t = 0; t < nc; ++t) { // every entry of the totally symmetric tensor from its one sum
            int ix[4] = {elas_ca(D, s), elas_cb(D, s), elas_ca(D, t), elas_cb(D, t)};
            std::sort(ix, ix + 4);
            born[s * nc + t] = hsum[nc + elas_born_index(D, ix[0], ix[1], ix[2], ix[3])];
        }
    E.epoch = ctx->hess.epoch;
    API_END
}

int md_elas_solve(md_ctx *ctx, double tol, int64_t max_iter, int64_t *iters, double *resid, double *xi_norm, int *status,
                  double *nonaffine, double *u)
{
    API_BEGIN
    elas_of(ctx, "md_elas_solve", true);
    if (!(tol > 0.0) || !std::isfinite(tol)) throw HipError("md_elas_solve: tol must be > 0");
    if (max_iter < 1 || max_iter > 0x3fffffff) throw HipError("md_elas_solve: max_iter must be in 1..1073741823");
    if (!iters || !resid || !xi_norm || !status || !nonaffine)
        throw HipError("md_elas_solve: iters / resid / xi_norm / status / nonaffine is null");
    if (ctx->dim == 3)
        elas_solve_t<3>(ctx, tol, max_iter, iters, resid, xi_norm, status, nonaffine, u);
    else
        elas_solve_t<2>(ctx, tol, max_iter, iters, resid, xi_norm, status, nonaffine, u);
    API_END
}

// ---------------------------------------------------------------------------------------------
// Cell changes of a live handle and the non-affine displacement since a mark (md_cell.hpp)
static NaffCell naff_cell(const md_ctx *ctx)
{
    NaffCell c{};
    c.tric = ctx->tric;
    for (int i = 0; i < 9; ++i) {
        c.a[i] = ctx->A[i];
        c.inv[i] = ctx->Ainv[i];
    }
    return c;
}

// the grid of a pair-walk sampler (md_rdf_, md_mpc_) in the new cell, its cell ranges and sort scratch grown to fit
static const auto regrid_pair_walk = [](md_ctx *c, auto &R, const char *who) {
    const RdfGrid g = pair_walk_grid(c, who, R.r_max);
    R.cell_start.ensure((size_t)g.ncell + 1);
    R.cell_end.ensure((size_t)g.ncell + 1);
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, R.keys_in.p, R.keys_out.p, R.vals_in.p, R.vals_out.p,
                                     (size_t)c->n, 0u, (unsigned)std::max(1, ceil_log2((uint64_t)g.ncell)), c->stream));
    R.sort_tmp.ensure(tmp_bytes);
    R.grid = g;
};

int md_set_cell(md_ctx *ctx, const double *box, int mode)
{
    API_BEGIN
    if (mode != MD_CELL_AFFINE && mode != MD_CELL_LATTICE) throw HipError("md_set_cell: mode must be MD_CELL_AFFINE or MD_CELL_LATTICE");
    if (!box) throw HipError("md_set_cell: box is null");
    if (ctx->dom.on) throw HipError("md_set_cell: not available on a slab-decomposition handle");
    require_state(ctx, "md_set_cell");
    if (ctx->snap_pending) throw HipError("md_set_cell: a frame is in flight (collect it with md_snapshot_end first)");
    const char *holder = ctx->dyn.on ? "md_dyn" : ctx->sq.on ? "md_sq" : ctx->current.on ? "md_cur" : ctx->chi4.on ? "md_chi4"
                         : ctx->cage.on ? "md_cage" : nullptr;
    if (holder)
        throw HipError(std::string("md_set_cell: the ") + holder + "_ sampler is set up on this handle; its stored origins or "
                       "wave vectors belong to the cell it was set up in");
    const int dim = ctx->dim;
    CellGeom cg;
    if (const char *why = cell_geometry(dim, box, cg)) {
        std::string w(why);
        throw HipError("md_set_cell" + w.substr(w.find(':')));
    }
    for (int c = 0; c < dim; ++c)
        if (cg.perp[c] / 3.0 < ctx->rc) {
            char b[320];
            snprintf(b, sizeof b,
                     "md_set_cell: the new cell is too small for the linked-cell build: the face distance %.17g of lattice "
                     "direction %d must be >= 3*list_cutoff = %.17g",
                     cg.perp[c], c, 3.0 * ctx->rc);
            throw HipError(b);
        }
    CellMap m{};
    m.tric_old = ctx->tric;
    m.tric_new = cg.tric;
    for (int i = 0; i < 9; ++i) {
        m.inv_old[i] = ctx->Ainv[i];
        m.a_new[i] = cg.A[i];
        m.inv_new[i] = cg.Ainv[i];
        m.minv[i] = (i % 4 == 0) ? 1 : 0;
    }
    if (mode == MD_CELL_LATTICE) {
        // M = U_old^-1 U_new: integer, unimodular, and U_old M = U_new again
        long long M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int r = 0; r < dim; ++r)
            for (int c = 0; c < dim; ++c) {
                double v = 0.0;
                for (int k = 0; k < dim; ++k) v += ctx->Ainv[r * 3 + k] * cg.A[k * 3 + c];
                const double q = std::nearbyint(v);
                if (!(std::fabs(v - q) <= 1e-9) || std::fabs(q) > 1024.0) {
                    char b[256];
                    snprintf(b, sizeof b, "md_set_cell: MD_CELL_LATTICE needs U_old^-1 U_new integer (entries up to 2^10); entry (%d, %d) is %.17g", r, c, v);
                    throw HipError(b);
                }
                M[r * 3 + c] = (long long)q;
            }
        const long long c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
        const long long det = M[0] * c00 + M[1] * c01 + M[2] * c02;
        if (det != 1 && det != -1) {
            char b[200];
            snprintf(b, sizeof b, "md_set_cell: MD_CELL_LATTICE needs |det(U_old^-1 U_new)| = 1, got %lld: the new cell generates another lattice", det);
            throw HipError(b);
        }
        for (int r = 0; r < dim; ++r)
            for (int c = 0; c < dim; ++c) {
                double v = 0.0, scale = 0.0;
                for (int k = 0; k < dim; ++k) {
                    v += ctx->A[r * 3 + k] * (double)M[k * 3 + c];
                    scale = std::max(scale, std::fabs(ctx->A[r * 3 + k] * (double)M[k * 3 + c]));
                }
                if (!(std::fabs(v - cg.A[r * 3 + c]) <= 8.0 * 2.220446049250313e-16 * scale))
                    throw HipError("md_set_cell: MD_CELL_LATTICE: U_old M does not give back the new cell; the new cell generates another lattice");
            }
        // the integer inverse: adjugate times det (det = +-1).  |M| <= 2^10 keeps its entries below 2^21, so that M^-1 img
        // (three terms of at most 2^21 2^31) stays far inside 64 bits in the kernel
        m.minv[0] = det * c00;
        m.minv[1] = det * (M[2] * M[7] - M[1] * M[8]);
        m.minv[2] = det * (M[1] * M[5] - M[2] * M[4]);
        m.minv[3] = det * c01;
        m.minv[4] = det * (M[0] * M[8] - M[2] * M[6]);
        m.minv[5] = det * (M[2] * M[3] - M[0] * M[5]);
        m.minv[6] = det * c02;
        m.minv[7] = det * (M[1] * M[6] - M[0] * M[7]);
        m.minv[8] = det * (M[0] * M[4] - M[1] * M[3]);
    }
    hipStream_t st = ctx->stream;
    md_ctx::Naff &Q = ctx->naff;
    const int n = (int)ctx->n, nb = ctx->nblk;
    double *mf = Q.marked ? Q.frac.p : nullptr;
    int32_t *mi = Q.marked ? Q.img.p : nullptr;
    auto launch = [&](int commit) {
        DevState s = ctx->dev(ctx->cur);
        if (mode == MD_CELL_AFFINE) {
            if (dim == 3)
                k_set_cell<3, MD_CELL_AFFINE_MODE><<<nb, MD_BLOCK, 0, st>>>(n, s, m, commit, Q.range_error.p, mf, mi);
            else
                k_set_cell<2, MD_CELL_AFFINE_MODE><<<nb, MD_BLOCK, 0, st>>>(n, s, m, commit, Q.range_error.p, mf, mi);
        } else {
            if (dim == 3)
                k_set_cell<3, MD_CELL_LATTICE_MODE><<<nb, MD_BLOCK, 0, st>>>(n, s, m, commit, Q.range_error.p, mf, mi);
            else
                k_set_cell<2, MD_CELL_LATTICE_MODE><<<nb, MD_BLOCK, 0, st>>>(n, s, m, commit, Q.range_error.p, mf, mi);
        }
        HIPCHK(hipGetLastError());
    };
    if (mode == MD_CELL_LATTICE) {
        Q.range_error.ensure(1);
        HIPCHK(hipMemsetAsync(Q.range_error.p, 0, sizeof(int), st));
        launch(0);
        int bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, Q.range_error.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (bad) throw HipError("md_set_cell: MD_CELL_LATTICE: an image count would leave the int32 range in the new basis");
    }
    // the host side first, so that a refusal from the grids leaves the particles where they are
    struct Saved {
        double L[3], A[9], Ainv[9], perp[3], volume, skin, rl;
        int tric, ncell_ext;
        BoxGrid grid;
        bool list_valid;
    } old;
    for (int c = 0; c < 3; ++c) old.L[c] = ctx->L[c], old.perp[c] = ctx->perp[c];
    for (int c = 0; c < 9; ++c) old.A[c] = ctx->A[c], old.Ainv[c] = ctx->Ainv[c];
    old.volume = ctx->volume, old.skin = ctx->skin, old.rl = ctx->rl, old.tric = ctx->tric, old.ncell_ext = ctx->ncell_ext;
    old.grid = ctx->grid, old.list_valid = ctx->list_valid;
    auto put = [&](const double *L, const double *A, const double *Ainv, const double *perp, double volume, int tric) {
        for (int c = 0; c < 3; ++c) ctx->L[c] = L[c], ctx->perp[c] = perp[c];
        for (int c = 0; c < 9; ++c) ctx->A[c] = A[c], ctx->Ainv[c] = Ainv[c];
        ctx->volume = volume;
        ctx->tric = tric;
    };
    double Lnew[3] = {1, 1, 1};
    for (int c = 0; c < dim; ++c) Lnew[c] = cg.A[c * 3 + c];
    put(Lnew, cg.A, cg.Ainv, cg.perp, cg.volume, cg.tric);
    const RdfGrid old_rdf = ctx->rdf.grid, old_mpc = ctx->mpc.grid;
    const double4 *old_pos[2] = {ctx->sb[0].pos.p, ctx->sb[1].pos.p};
    const bool old_stale = ctx->grid_stale; // (md_scale_cell: the grid put back below may still be owed to a build)
    try {
        configure_grid(ctx);
        if (ctx->rdf.on) regrid_pair_walk(ctx, ctx->rdf, "md_set_cell (md_rdf_ sampler)");
        if (ctx->mpc.on) regrid_pair_walk(ctx, ctx->mpc, "md_set_cell (md_mpc_ sampler)");
        // capacities after the new grid and density, as create_common and md_set_skin derive them (buffers only grow; the
        // rows are allocated aside and swapped in, so that a failed allocation leaves the old ones in place)
        double frac = 1.0;
        for (int c = 0; c < dim; ++c) frac *= (double)ctx->grid.ncx[c] / ctx->grid.nc[c];
        const int64_t gcap = (int64_t)((frac - 1.0) * 1.3 * ctx->ncap) + 4096;
        ensure_capacity(ctx, ctx->ncap + gcap);
        double dens = (double)ctx->n_global;
        dens /= ctx->volume;
        double vol = (dim == 3) ? 4.18879020478639 * ctx->rl * ctx->rl * ctx->rl : 3.14159265358979 * ctx->rl * ctx->rl;
        int maxn = ((int)(dens * vol * 1.35) + 24 + 3) & ~3;
        if (maxn > ctx->maxn) {
            DBuf<uint32_t> rows;
            DBuf<uint16_t> rows16;
            rows.alloc((size_t)ctx->ntiles * maxn * 64);
            rows16.alloc((size_t)ctx->ntiles * maxn * 64);
            std::swap(ctx->nlist.p, rows.p);
            std::swap(ctx->nlist.n, rows.n);
            std::swap(ctx->nlist16.p, rows16.p);
            std::swap(ctx->nlist16.n, rows16.n);
            ctx->maxn = maxn;
            old.list_valid = false; // (the rows of the old list went with the old buffers)
        }
    } catch (...) {
        (void)hipGetLastError();
        put(old.L, old.A, old.Ainv, old.perp, old.volume, old.tric);
        ctx->skin = old.skin, ctx->rl = old.rl, ctx->ncell_ext = old.ncell_ext, ctx->grid = old.grid;
        // (a state buffer that was grown before the failure holds the owned particles only: the list's ghosts are gone)
        ctx->list_valid = old.list_valid && ctx->sb[0].pos.p == old_pos[0] && ctx->sb[1].pos.p == old_pos[1];
        ctx->rdf.grid = old_rdf, ctx->mpc.grid = old_mpc;
        ctx->grid_stale = old_stale;
        throw;
    }
    launch(1);
    ctx->list_valid = false;
    ctx->inner_valid = false;
    ctx->hess.frozen = false;
    ctx->target_interval = 8;
    ctx->rate_known = false;
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

// Isotropic scale of the whole frame that keeps the Verlet rows (md_baro.hpp).
int md_scale_cell(md_ctx *ctx, double mu, double vscale, int *rows_kept)
{
    API_BEGIN
    if (!std::isfinite(mu) || !(mu > 0.0)) throw HipError("md_scale_cell: mu must be finite and > 0");
    if (!std::isfinite(vscale)) throw HipError("md_scale_cell: vscale must be finite");
    if (ctx->dom.on) throw HipError("md_scale_cell: not available on a slab-decomposition handle");
    require_state(ctx, "md_scale_cell");
    if (ctx->snap_pending) throw HipError("md_scale_cell: a frame is in flight (collect it with md_snapshot_end first)");
    const char *holder = ctx->dyn.on ? "md_dyn" : ctx->sq.on ? "md_sq" : ctx->current.on ? "md_cur" : ctx->chi4.on ? "md_chi4"
                         : ctx->cage.on ? "md_cage" : nullptr;
    if (holder)
        throw HipError(std::string("md_scale_cell: the ") + holder + "_ sampler is set up on this handle; its stored origins or "
                       "wave vectors belong to the cell it was set up in");
    const int dim = ctx->dim;
    double box[9];
    {
#pragma clang fp contract(off)
        for (int c = 0; c < dim; ++c)
            for (int r = 0; r < dim; ++r) box[c * dim + r] = mu * ctx->A[r * 3 + c];
    }
    CellGeom cg;
    if (const char *why = cell_geometry(dim, box, cg)) {
        std::string w(why);
        throw HipError("md_scale_cell" + w.substr(w.find(':')));
    }
    for (int c = 0; c < dim; ++c) {
        const double need = std::max({ctx->rc, ctx->rdf.on ? ctx->rdf.r_max : 0.0, ctx->mpc.on ? ctx->mpc.r_max : 0.0});
        if (cg.perp[c] / 3.0 < ctx->rc || cg.perp[c] < 3.0 * need) {
            char b[360];
            snprintf(b, sizeof b,
                     "md_scale_cell: the new cell is too small: the face distance %.17g of lattice direction %d must be >= "
                     "3*list_cutoff = %.17g%s",
                     cg.perp[c], c, 3.0 * ctx->rc,
                     need > ctx->rc ? " and >= 3*r_max of the md_rdf_ / md_mpc_ sampler set up on this handle" : "");
            throw HipError(b);
        }
    }
    hipStream_t st = ctx->stream;
    ctx->scale_dmax.ensure(MD_SCALE_NOUT);
    // the host side first, so that a refusal from the samplers' grids leaves the particles where they are.  The cell grid
    // of the list is NOT derived again: the live rows' ghost slots and halo lists belong to it (rebuild() does, later);
    // only the periodic translations in it follow now -- the exports and the ghost refresh read them.
    struct Saved {
        double L[3], A[9], Ainv[9], perp[3], volume;
        BoxGrid grid;
        RdfGrid rdf, mpc;
    } old;
    for (int c = 0; c < 3; ++c) old.L[c] = ctx->L[c], old.perp[c] = ctx->perp[c];
    for (int c = 0; c < 9; ++c) old.A[c] = ctx->A[c], old.Ainv[c] = ctx->Ainv[c];
    old.volume = ctx->volume, old.grid = ctx->grid, old.rdf = ctx->rdf.grid, old.mpc = ctx->mpc.grid;
    for (int c = 0; c < dim; ++c) ctx->L[c] = cg.A[c * 3 + c];
    for (int c = 0; c < 3; ++c) ctx->perp[c] = cg.perp[c];
    for (int c = 0; c < 9; ++c) ctx->A[c] = cg.A[c], ctx->Ainv[c] = cg.Ainv[c];
    ctx->volume = cg.volume;
    try {
        if (ctx->rdf.on) regrid_pair_walk(ctx, ctx->rdf, "md_scale_cell (md_rdf_ sampler)");
        if (ctx->mpc.on) regrid_pair_walk(ctx, ctx->mpc, "md_scale_cell (md_mpc_ sampler)");
    } catch (...) {
        (void)hipGetLastError();
        for (int c = 0; c < 3; ++c) ctx->L[c] = old.L[c], ctx->perp[c] = old.perp[c];
        for (int c = 0; c < 9; ++c) ctx->A[c] = old.A[c], ctx->Ainv[c] = old.Ainv[c];
        ctx->volume = old.volume, ctx->rdf.grid = old.rdf, ctx->mpc.grid = old.mpc;
        throw;
    }
    BoxGrid &g = ctx->grid;
    for (int c = 0; c < dim; ++c) {
        g.L[c] = ctx->L[c];
        g.invL[c] = 1.0 / ctx->L[c];
    }
    for (int c = 0; c < 9; ++c) g.A[c] = ctx->A[c], g.Ainv[c] = ctx->Ainv[c];
    ctx->grid_stale = true;
    ctx->hess.frozen = false;

    // Which rows can stay.  The tiled two-level rows of a built-in potential; anything else (user potentials, skin 0, rows
    // that did not fit LDS) is scaled and builds again.  Floor: a kept list must leave at least two thirds of the configured
    // skin (inner skin).  The steps a list lasts are proportional to the skin it has left; couplings of a barostat move it
    // by parts in a thousand, so a list that has lost a third of its skin has been compressed by hand, and the build it
    // saves would come a third sooner anyway.  (A non-positive skin covers nothing.)
    bool keep = ctx->list_valid && ctx->use_tiles && ctx->skin > 0.0 && ctx->pot_kind != POT_CUSTOM;
    const double m0n = ctx->m0 * mu, m1n = ctx->m1 * mu;
    // (a list md_deform_cell has mapped carries its singular-value bound along; one that was only scaled: the doubles as ever)
    const double se = ctx->deformed0 ? (m0n * ctx->ds0) * ctx->rl - ctx->rc : m0n * ctx->rl - ctx->rc;
    const double ie = ctx->deformed1 ? (m1n * ctx->ds1) * (ctx->rc + ctx->inner_skin) - ctx->rc
                                     : m1n * (ctx->rc + ctx->inner_skin) - ctx->rc;
    if (keep && !(se >= (2.0 / 3.0) * ctx->skin)) keep = false;
    bool keep_in = keep && ctx->inner_valid;
    if (keep_in && !(ie >= (2.0 / 3.0) * ctx->inner_skin)) keep_in = false;
    if (!keep_in) ctx->inner_valid = false; // (dev(): x1 aliases x0 from here on; the next step prunes, or builds)
    const int n = (int)ctx->n;
    const int npos = (keep && !ctx->virtual_ghosts) ? (int)ctx->next : n; // real ghost records go along with their rows
    const double half_skin = keep ? 0.5 * se : INFINITY, half_inner = keep_in ? 0.5 * ie : INFINITY;
    unsigned long long hb[MD_SCALE_NOUT] = {0ull, 0ull, 0ull};
    // From here on the host holds the new cell: a HIP error in the pass or its read-back leaves it unknown whether the
    // particles went along.  No list is valid then, and every entry that reads the state refuses until a full md_upload
    // replaces it (state_invalid, as after a failed step loop).
    try {
        HIPCHK(hipMemsetAsync(ctx->scale_dmax.p, 0, MD_SCALE_NOUT * sizeof(unsigned long long), st));
        if (npos > 0) {
            DevState s = ctx->dev(ctx->cur);
            const int has_x1 = keep_in ? 1 : 0;
            if (dim == 3)
                k_scale_cell<3><<<nblocks(npos), MD_BLOCK, 0, st>>>(n, npos, s, mu, vscale, has_x1, half_skin, half_inner,
                                                                    ctx->scal.p, ctx->scale_dmax.p);
            else
                k_scale_cell<2><<<nblocks(npos), MD_BLOCK, 0, st>>>(n, npos, s, mu, vscale, has_x1, half_skin, half_inner,
                                                                    ctx->scal.p, ctx->scale_dmax.p);
            if (keep_in) k_scale_commit<<<1, 1, 0, st>>>(ctx->scal.p, ctx->scale_dmax.p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(hb, ctx->scale_dmax.p, sizeof hb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } catch (...) {
        ctx->list_valid = ctx->inner_valid = false;
        ctx->m0 = ctx->m1 = 1.0;
        ctx->scaled0 = ctx->scaled1 = false;
        deform_reset0(ctx), deform_reset1(ctx);
        ctx->state_invalid = true;
        throw;
    }
    double dsq[MD_SCALE_NOUT];
    memcpy(dsq, hb, sizeof dsq);
    // the kernel's verdict (k_kickdrift's criterion): dsq[0], dsq[1] are zero unless a particle lies beyond half_skin of
    // its x0 -- what md_compute_forces and a prune step walk the outer rows on -- or beyond min(half_inner, half_skin - d1)
    // of its x1; dsq[2] is the d1^2 the kernel formed that limit from
    if (keep && !(dsq[0] <= half_skin * half_skin)) keep = false;
    if (keep && keep_in) {
        const double thr = std::fmin(half_inner, half_skin - std::sqrt(dsq[2]));
        if (!(thr > 0.0 && dsq[1] <= thr * thr)) keep_in = false;
    }
    if (keep) {
        ctx->m0 = m0n;
        ctx->scaled0 = true;
        if (keep_in) {
            ctx->m1 = m1n;
            ctx->scaled1 = true;
        } else {
            ctx->inner_valid = false;
        }
    } else {
        ctx->list_valid = false;
        ctx->inner_valid = false;
    }
    if (!ctx->inner_valid) ctx->m1 = 1.0, ctx->scaled1 = false, deform_reset1(ctx);
    if (!ctx->list_valid) ctx->m0 = 1.0, ctx->scaled0 = false, deform_reset0(ctx);
    if (rows_kept) *rows_kept = keep ? 1 : 0;
    API_END
}

// General affine map of the whole frame that keeps the Verlet rows (md_deform.hpp).
namespace {

// Extreme eigenvalues of the symmetric d x d matrix C (row-major 3 x 3, d <= 3) by cyclic Jacobi rotations: each rotation
// is orthogonal to rounding, the off-diagonal mass falls quadratically; ten sweeps leave it below 1e-30 of the trace.
void sym_eig_minmax(const double *Cin, int d, double &lmin, double &lmax)
{
    double a[9];
    for (int i = 0; i < 9; ++i) a[i] = Cin[i];
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0, tr = 0.0;
        for (int p = 0; p < d; ++p) {
            tr += std::fabs(a[p * 3 + p]);
            for (int q = p + 1; q < d; ++q) off += a[p * 3 + q] * a[p * 3 + q];
        }
        if (!(off > 1e-60 * tr * tr)) break;
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q) {
                const double apq = a[p * 3 + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * 3 + q] - a[p * 3 + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < d; ++k) { // columns p, q
                    const double akp = a[k * 3 + p], akq = a[k * 3 + q];
                    a[k * 3 + p] = cs * akp - sn * akq;
                    a[k * 3 + q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < d; ++k) { // rows p, q
                    const double apk = a[p * 3 + k], aqk = a[q * 3 + k];
                    a[p * 3 + k] = cs * apk - sn * aqk;
                    a[q * 3 + k] = sn * apk + cs * aqk;
                }
            }
    }
    lmin = lmax = a[0];
    for (int p = 1; p < d; ++p) lmin = std::min(lmin, a[p * 3 + p]), lmax = std::max(lmax, a[p * 3 + p]);
}

// lo <= sigma_min(M), hi >= sigma_max(M): the singular values from the eigenproblem of M^T M, widened by a relative 2^-40
// in the safe direction (the product, the rotations and the root err by a few 2^-52 of sigma_max^2; for the maps rows
// survive -- condition numbers within a few per cent of 1 -- that is twelve bits inside the margin).
void singular_bounds(const double *M, int d, double &lo, double &hi)
{
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c) {
            double v = 0.0;
            for (int k = 0; k < d; ++k) v += M[k * 3 + r] * M[k * 3 + c];
            C[r * 3 + c] = v;
        }
    double l0, l1;
    sym_eig_minmax(C, d, l0, l1);
    lo = std::sqrt(std::max(l0, 0.0)) * (1.0 - 0x1p-40);
    hi = std::sqrt(std::max(l1, 0.0)) * (1.0 + 0x1p-40);
}

// (every product and sum rounded, k ascending: a test restates the product of its own F's bit for bit)
void mat3_mul(const double *A, const double *B, int d, double *out) // out = A B (row-major 3 x 3, upper left d x d)
{
#pragma clang fp contract(off)
    double t[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c) {
            double v = 0.0;
            for (int k = 0; k < d; ++k) v += A[r * 3 + k] * B[k * 3 + c];
            t[r * 3 + c] = v;
        }
    for (int i = 0; i < 9; ++i) out[i] = t[i];
}

} // namespace

int md_deform_cell(md_ctx *ctx, const double *F, const double *G, int *rows_kept)
{
    API_BEGIN
    if (!F) throw HipError("md_deform_cell: F is null");
    const int dim = ctx->dim;
    DeformMap m{};
    for (int i = 0; i < 9; ++i) m.F[i] = m.G[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int r = 0; r < dim; ++r)
        for (int c = 0; c < dim; ++c) {
            m.F[r * 3 + c] = F[r * dim + c];
            if (G) m.G[r * 3 + c] = G[r * dim + c];
            if (!std::isfinite(m.F[r * 3 + c])) throw HipError("md_deform_cell: the entries of F must be finite");
            if (!std::isfinite(m.G[r * 3 + c])) throw HipError("md_deform_cell: the entries of G must be finite");
        }
    {
        const double *f = m.F;
        const double det = f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) + f[2] * (f[3] * f[7] - f[4] * f[6]);
        if (!(det > 0.0) || !std::isfinite(det)) throw HipError("md_deform_cell: det F must be finite and > 0");
    }
    if (ctx->dom.on) throw HipError("md_deform_cell: not available on a slab-decomposition handle");
    require_state(ctx, "md_deform_cell");
    if (ctx->snap_pending) throw HipError("md_deform_cell: a frame is in flight (collect it with md_snapshot_end first)");
    const char *holder = ctx->dyn.on ? "md_dyn" : ctx->sq.on ? "md_sq" : ctx->current.on ? "md_cur" : ctx->chi4.on ? "md_chi4"
                         : ctx->cage.on ? "md_cage" : nullptr;
    if (holder)
        throw HipError(std::string("md_deform_cell: the ") + holder + "_ sampler is set up on this handle; its stored origins or "
                       "wave vectors belong to the cell it was set up in");
    double box[9];
    {
#pragma clang fp contract(off)
        // F U, row times column, left to right, every product and sum rounded (numpy restates it entry by entry)
        for (int c = 0; c < dim; ++c)
            for (int r = 0; r < dim; ++r) {
                double t = m.F[r * 3 + 0] * ctx->A[0 * 3 + c] + m.F[r * 3 + 1] * ctx->A[1 * 3 + c];
                if (dim == 3) t = t + m.F[r * 3 + 2] * ctx->A[2 * 3 + c];
                box[c * dim + r] = t;
            }
    }
    CellGeom cg;
    if (const char *why = cell_geometry(dim, box, cg)) {
        std::string w(why);
        throw HipError("md_deform_cell" + w.substr(w.find(':')));
    }
    for (int c = 0; c < dim; ++c) {
        const double need = std::max({ctx->rc, ctx->rdf.on ? ctx->rdf.r_max : 0.0, ctx->mpc.on ? ctx->mpc.r_max : 0.0});
        if (cg.perp[c] / 3.0 < ctx->rc || cg.perp[c] < 3.0 * need) {
            char b[360];
            snprintf(b, sizeof b,
                     "md_deform_cell: the new cell is too small: the face distance %.17g of lattice direction %d must be >= "
                     "3*list_cutoff = %.17g%s",
                     cg.perp[c], c, 3.0 * ctx->rc,
                     need > ctx->rc ? " and >= 3*r_max of the md_rdf_ / md_mpc_ sampler set up on this handle" : "");
            throw HipError(b);
        }
    }
    // the singular-value bounds of this call's F and of the accumulated maps (host arithmetic only: nothing is committed)
    double Fs, FS, M0n[9], M1n[9], s0n, S0n, s1n, S1n;
    singular_bounds(m.F, dim, Fs, FS);
    mat3_mul(m.F, ctx->Md0, dim, M0n);
    mat3_mul(m.F, ctx->Md1, dim, M1n);
    singular_bounds(M0n, dim, s0n, S0n);
    singular_bounds(M1n, dim, s1n, S1n);
    if (!(Fs > 0.0) || !(s0n > 0.0) || !(s1n > 0.0) || !std::isfinite(FS))
        throw HipError("md_deform_cell: F is singular to working precision");

    hipStream_t st = ctx->stream;
    ctx->scale_dmax.ensure(MD_SCALE_NOUT);
    // the host side first, as md_scale_cell: a refusal from the samplers' grids leaves the particles where they are; the
    // cell grid of the list is not derived again (rebuild() does), only its periodic translations follow now
    struct Saved {
        double L[3], A[9], Ainv[9], perp[3], volume;
        int tric;
        RdfGrid rdf, mpc;
    } old;
    for (int c = 0; c < 3; ++c) old.L[c] = ctx->L[c], old.perp[c] = ctx->perp[c];
    for (int c = 0; c < 9; ++c) old.A[c] = ctx->A[c], old.Ainv[c] = ctx->Ainv[c];
    old.volume = ctx->volume, old.tric = ctx->tric, old.rdf = ctx->rdf.grid, old.mpc = ctx->mpc.grid;
    for (int c = 0; c < dim; ++c) ctx->L[c] = cg.A[c * 3 + c];
    for (int c = 0; c < 3; ++c) ctx->perp[c] = cg.perp[c];
    for (int c = 0; c < 9; ++c) ctx->A[c] = cg.A[c], ctx->Ainv[c] = cg.Ainv[c];
    ctx->volume = cg.volume;
    ctx->tric = cg.tric;
    try {
        if (ctx->rdf.on) regrid_pair_walk(ctx, ctx->rdf, "md_deform_cell (md_rdf_ sampler)");
        if (ctx->mpc.on) regrid_pair_walk(ctx, ctx->mpc, "md_deform_cell (md_mpc_ sampler)");
    } catch (...) {
        (void)hipGetLastError();
        for (int c = 0; c < 3; ++c) ctx->L[c] = old.L[c], ctx->perp[c] = old.perp[c];
        for (int c = 0; c < 9; ++c) ctx->A[c] = old.A[c], ctx->Ainv[c] = old.Ainv[c];
        ctx->volume = old.volume, ctx->tric = old.tric, ctx->rdf.grid = old.rdf, ctx->mpc.grid = old.mpc;
        throw;
    }
    BoxGrid &g = ctx->grid;
    for (int c = 0; c < dim; ++c) {
        g.L[c] = ctx->L[c];
        g.invL[c] = 1.0 / ctx->L[c];
    }
    for (int c = 0; c < 9; ++c) g.A[c] = ctx->A[c], g.Ainv[c] = ctx->Ainv[c];
    g.tric = ctx->tric;
    ctx->grid_stale = true;
    ctx->hess.frozen = false;

    // Which rows can stay: md_scale_cell's rule, and the cell must stay of its kind -- tric selects code paths in the
    // kernels that read the live rows (shift codes of a diagonal cell are box lengths, of a general one lattice vectors).
    bool keep = ctx->list_valid && ctx->use_tiles && ctx->skin > 0.0 && ctx->pot_kind != POT_CUSTOM && cg.tric == old.tric;
    const double se = (ctx->m0 * s0n) * ctx->rl - ctx->rc, ie = (ctx->m1 * s1n) * (ctx->rc + ctx->inner_skin) - ctx->rc;
    if (keep && !(se >= (2.0 / 3.0) * ctx->skin)) keep = false;
    bool keep_in = keep && ctx->inner_valid;
    if (keep_in && !(ie >= (2.0 / 3.0) * ctx->inner_skin)) keep_in = false;
    if (!keep_in) ctx->inner_valid = false; // (dev(): x1 aliases x0 from here on; the next step prunes, or builds)
    const int n = (int)ctx->n;
    const int npos = (keep && !ctx->virtual_ghosts) ? (int)ctx->next : n; // real ghost records go along with their rows
    const double half_skin = keep ? 0.5 * se : INFINITY, half_inner = keep_in ? 0.5 * ie : INFINITY;
    unsigned long long hb[MD_SCALE_NOUT] = {0ull, 0ull, 0ull};
    // From here on the host holds the new cell: a HIP error leaves it unknown whether the particles went along
    // (state_invalid, as md_scale_cell).
    try {
        HIPCHK(hipMemsetAsync(ctx->scale_dmax.p, 0, MD_SCALE_NOUT * sizeof(unsigned long long), st));
        if (npos > 0) {
            DevState s = ctx->dev(ctx->cur);
            const int has_x1 = keep_in ? 1 : 0, has_g = G ? 1 : 0;
            if (dim == 3)
                k_deform_cell<3><<<nblocks(npos), MD_BLOCK, 0, st>>>(n, npos, s, m, has_g, has_x1, half_skin, half_inner, FS,
                                                                     ctx->scal.p, ctx->scale_dmax.p);
            else
                k_deform_cell<2><<<nblocks(npos), MD_BLOCK, 0, st>>>(n, npos, s, m, has_g, has_x1, half_skin, half_inner, FS,
                                                                     ctx->scal.p, ctx->scale_dmax.p);
            if (keep_in) k_scale_commit<<<1, 1, 0, st>>>(ctx->scal.p, ctx->scale_dmax.p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(hb, ctx->scale_dmax.p, sizeof hb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } catch (...) {
        ctx->list_valid = ctx->inner_valid = false;
        ctx->m0 = ctx->m1 = 1.0;
        ctx->scaled0 = ctx->scaled1 = false;
        deform_reset0(ctx), deform_reset1(ctx);
        ctx->state_invalid = true;
        throw;
    }
    double dsq[MD_SCALE_NOUT];
    memcpy(dsq, hb, sizeof dsq);
    if (keep && !(dsq[0] <= half_skin * half_skin)) keep = false;
    if (keep && keep_in) {
        const double thr = std::fmin(half_inner, half_skin - std::sqrt(dsq[2]));
        if (!(thr > 0.0 && dsq[1] <= thr * thr)) keep_in = false;
    }
    if (keep) {
        for (int i = 0; i < 9; ++i) ctx->Md0[i] = M0n[i];
        ctx->ds0 = s0n, ctx->dS0 = S0n;
        ctx->deformed0 = true;
        if (keep_in) {
            for (int i = 0; i < 9; ++i) ctx->Md1[i] = M1n[i];
            ctx->ds1 = s1n, ctx->dS1 = S1n;
            ctx->deformed1 = true;
        } else {
            ctx->inner_valid = false;
        }
    } else {
        ctx->list_valid = false;
        ctx->inner_valid = false;
    }
    if (!ctx->inner_valid) ctx->m1 = 1.0, ctx->scaled1 = false, deform_reset1(ctx);
    if (!ctx->list_valid) ctx->m0 = 1.0, ctx->scaled0 = false, deform_reset0(ctx);
    if (rows_kept) *rows_kept = keep ? 1 : 0;
    API_END
}

int md_deform_state(md_ctx *ctx, double *m0, double *m1, double *sig)
{
    API_BEGIN
    // (md_scale_cell's scalars are part of the accumulated maps: a handle that was only scaled reports mu 1)
    const bool v0 = ctx->list_valid, v1 = ctx->list_valid && ctx->inner_valid;
    const double a0 = v0 ? ctx->m0 : 1.0, a1 = v1 ? ctx->m1 : 1.0;
    for (int i = 0; i < 9; ++i) {
        const double id = (i % 4 == 0) ? 1.0 : 0.0;
        const bool used = i / 3 < ctx->dim && i % 3 < ctx->dim; // (2-D: the third row and column stay those of the identity)
        if (m0) m0[i] = used ? a0 * ((v0 && ctx->deformed0) ? ctx->Md0[i] : id) : id;
        if (m1) m1[i] = used ? a1 * ((v1 && ctx->deformed1) ? ctx->Md1[i] : id) : id;
    }
    if (sig) {
        const bool d0 = v0 && ctx->deformed0, d1 = v1 && ctx->deformed1;
        sig[0] = d0 ? a0 * ctx->ds0 : a0;
        sig[1] = d0 ? a0 * ctx->dS0 : a0;
        sig[2] = d1 ? a1 * ctx->ds1 : a1;
        sig[3] = d1 ? a1 * ctx->dS1 : a1;
    }
    API_END
}

int md_nonaffine_mark(md_ctx *ctx)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_nonaffine_mark: not available on a slab-decomposition handle");
    require_state(ctx, "md_nonaffine_mark");
    md_ctx::Naff &Q = ctx->naff;
    const size_t nd = (size_t)ctx->n * ctx->dim;
    Q.marked = false;
    Q.frac.ensure(nd);
    Q.img.ensure(nd);
    DevState s = ctx->dev(ctx->cur);
    if (ctx->dim == 3)
        k_naff_mark<3><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, naff_cell(ctx), Q.frac.p, Q.img.p);
    else
        k_naff_mark<2><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, naff_cell(ctx), Q.frac.p, Q.img.p);
    HIPCHK(hipGetLastError());
    Q.marked = true;
    API_END
}

int md_nonaffine(md_ctx *ctx, double *sums, double *u)
{
    API_BEGIN
    if (ctx->dom.on) throw HipError("md_nonaffine: not available on a slab-decomposition handle");
    require_state(ctx, "md_nonaffine");
    md_ctx::Naff &Q = ctx->naff;
    if (!Q.marked)
        throw HipError("md_nonaffine: no mark (call md_nonaffine_mark first; an md_upload of positions discards the mark)");
    if (!sums) throw HipError("md_nonaffine: sums is null");
    const size_t nd = (size_t)ctx->n * ctx->dim;
    const int nb = ctx->nblk;
    hipStream_t st = ctx->stream;
    if (u) Q.u.ensure(nd);
    Q.part.ensure((size_t)MD_NAFF_NSUM * nb);
    Q.pmax.ensure(nb);
    Q.pid.ensure(nb);
    Q.gmax.ensure(1);
    Q.out.ensure(8);
    HIPCHK(hipMemsetAsync(Q.gmax.p, 0, sizeof(unsigned long long), st));
    DevState s = ctx->dev(ctx->cur);
    double *uo = u ? Q.u.p : nullptr;
    if (ctx->dim == 3)
        k_naff<3><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, naff_cell(ctx), Q.frac.p, Q.img.p, uo, Q.part.p, Q.pmax.p, Q.pid.p, Q.gmax.p);
    else
        k_naff<2><<<nb, MD_BLOCK, 0, st>>>((int)ctx->n, s, naff_cell(ctx), Q.frac.p, Q.img.p, uo, Q.part.p, Q.pmax.p, Q.pid.p, Q.gmax.p);
    k_naff_finish<<<MD_NAFF_NSUM + 1, MD_BLOCK, 0, st>>>(nb, (int)ctx->n, Q.part.p, Q.pmax.p, Q.pid.p, Q.gmax.p, Q.out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, Q.out.p, sizeof(double) * 8, hipMemcpyDeviceToHost, st));
    if (u) HIPCHK(hipMemcpyAsync(u, Q.u.p, sizeof(double) * nd, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

static void debug_tile_halos(md_ctx *ctx);
int md_run(md_ctx *ctx, int64_t nsteps, double dt, int ensemble, double tau, double nf, const double *ktemp,
           const double *r1, const double *r2, double *uwk)
{
    API_BEGIN
    require_state(ctx, "md_run");
    if (nsteps < 0) throw HipError("md_run: nsteps must be >= 0");
    if (nsteps > 0x3fffffff) throw HipError("md_run: nsteps too large for one call");
    if (ensemble != MD_NVE && ensemble != MD_NVT) throw HipError("md_run: unknown ensemble");
    bool nvt = ensemble == MD_NVT;
    if (nvt && (!ktemp || !r1 || !r2)) throw HipError("md_run: NVT needs ktemp, r1 and r2 arrays");
    if (nvt && !(tau > 0.0)) throw HipError("md_run: NVT needs tau > 0");
    if (nsteps == 0) {
        if (uwk) uwk[0] = uwk[1] = uwk[2] = NAN;
        return 0;
    }
    hipStream_t st = ctx->stream;
    ctx->hess.frozen = false;
    double term1 = 0.0;
    if (nvt) {
        ctx->d_kt.ensure(nsteps);
        ctx->d_r1.ensure(nsteps);
        ctx->d_r2.ensure(nsteps);
        HIPCHK(hipMemcpyAsync(ctx->d_kt.p, ktemp, nsteps * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->d_r1.p, r1, nsteps * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->d_r2.p, r2, nsteps * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        term1 = std::exp(-(dt / tau));
    }
    if (!ctx->list_valid) rebuild(ctx);
    bool want = uwk != nullptr;
    auto force_part = [&](int t) {
        bool last = (t == (int)nsteps - 1);
        bool uw = last && want;
        launch_force(ctx, uw, true, dt, t);
        if (nvt || uw) launch_finalize(ctx, uw, nvt, nf, term1, t);
    };
    // The fused loop (k_step_tile: one launch per step) whenever the tiled rows exist; the
    // classic three-kernel sequence otherwise (slab handles, user potentials, rows that do not fit LDS, skin 0).
    bool fused = ctx->skin > 0.0 && fused_available(ctx);
    ctx->last_run_fused = fused;
    FusedScope fscope{ctx};
    fscope.done = !fused; // (the classic loop keeps the state in the arrays at every step boundary)
    if (fused) fused_enter(ctx, dt);
    auto step_part = [&](int t) {
        if (!fused) {
            launch_kickdrift(ctx, nvt, dt, true, t);
            launch_ghost_update(ctx, t);
            force_part(t);
            return;
        }
        bool last = (t == (int)nsteps - 1);
        bool uw = last && want;
        launch_step(ctx, uw, dt, t);
        if (nvt || uw) launch_finalize(ctx, uw, nvt, nf, term1, t);
    };
    // list build at a step boundary of the fused loop: records -> state arrays, build (permutes them), -> records
    auto fused_rebuild = [&]() {
        prof_begin(ctx, 2);
        fused_leave(ctx, false);
        fscope.done = true; // (the arrays hold the state of the last completed step)
        rebuild(ctx);
        fused = fused_available(ctx);
        if (fused) {
            fscope.done = false;
            fused_enter(ctx, dt);
        }
        prof_end(ctx);
    };
    if (ctx->skin <= 0.0) {
        // literal reference cadence: a fresh linked-cell build every step
        for (int t = 0; t < (int)nsteps; ++t) {
            launch_kickdrift(ctx, nvt, dt, false, t);
            rebuild(ctx);
            force_part(t);
        }
    } else {
        // Windows of steps are enqueued without host round-trips.  The drift kernel records the first
        // step at which a particle left the validity radius of the rows in use (`first_viol`); every
        // later kernel of the window skips itself, so speculation is safe and a window can span a whole
        // rebuild interval: one synchronisation per list build.
        //
        // With pruning on, the rows in use are the inner rows (cutoff + inner_skin): every L steps the force
        // evaluation is a prune step that rewrites them from the outer rows (cutoff + skin), and the outer
        // rows are rebuilt every R steps.  R and L follow from the measured growth rate of the largest
        // displacement (max_i |x_i - x_ref_i| grows ballistically, ~ rate * steps):
        //     rate * (R - 1) <= safety * skin/2          (outer rows valid at every step that uses them)
        //     1.1 * rate * (L - 1) <= safety * inner/2   (inner rows valid between two prunes)
        // with the segments evened out, L = ceil(R / ceil(R / Lmax)).  The device checks are the exact
        // criteria; the plan only has to make violations rare, and `safety` backs off when they happen.
        auto measure_disp0 = [&](double4 *pos_override = nullptr) -> double {
            k_reset_disp0<<<1, 1, 0, st>>>(ctx->scal.p);
            DevState sd = ctx->dev(ctx->cur);
            if (pos_override) sd.pos = pos_override;
            if (ctx->dim == 3)
                k_max_disp0<3><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, ctx->scal.p);
            else
                k_max_disp0<2><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, ctx->scal.p);
            Scalars h2 = read_scalars(ctx);
            double d0sq;
            unsigned long long bits = h2.max_disp2_bits;
            memcpy(&d0sq, &bits, sizeof d0sq);
            return std::sqrt(d0sq);
        };
        int s = 0;
        int redo_step = -1, redo_count = 0; // the same step violated again right after its list build
        std::vector<int> prune_steps;
        while (s < (int)nsteps) {
            const bool pruning = ctx->prune_on;
            int64_t R, L = INT64_MAX;
            if (!pruning) {
                R = ctx->target_interval;
            } else if (!ctx->rate_known) {
                R = ctx->steps_since_build + 4; // a short first window, measured at its end
                L = 4;
            } else {
                // (a system that has blown up measures NaN or inf displacements: plan the shortest windows -- the reference
                // goes on producing NaNs in that case, it does not stop; an unguarded NaN here ended in a SIGFPE of the
                // integer divisions below)
                double r_out = std::isfinite(ctx->d1_rate) ? std::max(ctx->d1_rate, 1e-12) : 1e300;
                double Rf = std::floor(ctx->safety * 0.5 * skin_eff(ctx) / r_out) + 1.0;
                double Lf = std::floor(ctx->safety * 0.5 * inner_eff(ctx) / (1.1 * r_out)) + 1.0;
                int64_t Rmax = (int64_t)std::min(std::max(Rf, 2.0), 4096.0);
                int64_t Lmax = (int64_t)std::min(std::max(Lf, 2.0), 4096.0);
                // a build costs about as much as 8 prune steps: take the R <= Rmax with the least
                // (build + prunes) per step -- a whole number of full segments often beats a ragged last one
                R = Rmax;
                double best = 1e300;
                for (int64_t r = std::max<int64_t>(2, Rmax - Lmax); r <= Rmax; ++r) {
                    double cost = (8.0 + (double)((r + Lmax - 1) / Lmax)) / (double)r;
                    if (cost <= best) {
                        best = cost;
                        R = r;
                    }
                }
                int64_t nseg = (R + Lmax - 1) / Lmax;
                L = (R + nseg - 1) / nseg;
            }
            int win_cap = (int)std::min<int64_t>(nsteps, (int64_t)s + std::max<int64_t>(1, R - ctx->steps_since_build));
            prune_steps.clear();
            int last_prune = -1;
            const int a_win = ctx->fz_a; // fused: the buffer set step s reads
            for (int t = s; t < win_cap; ++t) {
                if (pruning && ctx->inner_valid && ctx->steps_since_prune >= L)
                    ctx->inner_valid = false; // scheduled refresh of the inner rows
                if (pruning && !ctx->inner_valid) {
                    prune_steps.push_back(t);
                    last_prune = t;
                }
                step_part(t); // (a prune step marks the inner rows valid and zeroes steps_since_prune)
                ctx->steps_since_prune += 1;
            }
            int win_end = win_cap;
            HIPCHK(hipGetLastError());
            Scalars h = read_scalars(ctx);
            double d1 = 0.0;
            {
                unsigned long long bits = h.d1max2_bits;
                double d12;
                memcpy(&d12, &bits, sizeof d12);
                d1 = std::sqrt(d12);
            }
            if (getenv("MDHIP_TRACE_WINDOWS"))
                fprintf(stderr, "[mdhip] window %d..%d viol %d d1 %.4f rate %.5f safety %.3f since_build %lld R %lld L %lld nprune %zu\n",
                        s, win_end, h.first_viol < win_end ? h.first_viol : -1, d1, ctx->d1_rate, ctx->safety,
                        (long long)ctx->steps_since_build, (long long)R, (long long)(L == INT64_MAX ? -1 : L),
                        prune_steps.size());
            if (h.halo_overflow & 16) {
                // a tile's inner halo did not fit the LDS image planned for the ordinary steps: the prune step
                // recorded itself as violated; go on without inner halos (the list build below resets the flag)
                ctx->allow_inner_halo = false;
            }
            if (h.first_viol < win_end) {
                // everything from step m's force evaluation on was skipped on the device: refresh the
                // rows at the drifted positions and resume with the force half of step m
                int m = h.first_viol;
                // (fused loop: the step launched again after the previous violation can flag ITSELF -- its prune
                // found a tile whose inner halo does not fit -- which is seen only now: m == s - 1, nothing after it ran)
                if (m < s - 1 || (m < s && !fused)) throw HipError("internal: stale displacement-violation index");
                // The step launched again after a list build flags itself again: a particle moves more than half the
                // skin in ONE step (the rows of the fused loop are one step old when they are used).  Building again
                // cannot help and the loop would never advance: the run is beyond what a Verlet list can follow -- in
                // practice a system that has blown up.  (The reference rebuilds its cells every step and goes on printing
                // garbage; this is a stated deviation: an error instead.)
                if (m == redo_step) {
                    if (++redo_count >= 3)
                        throw HipError("md_run: a particle moves more than half the list skin in a single step (time step too "
                                       "large for this skin, or the system has blown up)");
                } else {
                    redo_step = m;
                    redo_count = 0;
                }
                ctx->st_viol++;
                bool m_was_prune = (h.halo_overflow & 16) != 0;
                for (int p : prune_steps)
                    if (p == m) m_was_prune = true;
                ctx->steps_since_build += (m - s) + 1;
                // fused loop: step m's launch read buffer set a_m and wrote the other one -- x_m included, which is
                // what the displacement is measured on; the state proper is still step m-1's, in set a_m
                const bool was_fused = fused;
                double4 *pos_m = nullptr;
                if (fused) {
                    ctx->fz_a = a_win ^ ((m - s) & 1);
                    pos_m = ctx->sb[ctx->cur ^ ctx->fz_a ^ 1].pos.p;
                }
                bool rebuilt;
                if (!pruning) {
                    int64_t observed = ctx->steps_since_build;
                    ctx->target_interval = std::max<int64_t>(2, (observed * 4) / 5);
                    if (fused)
                        fused_rebuild();
                    else
                        rebuild(ctx);
                    rebuilt = true;
                } else {
                    ctx->safety = std::max(0.5, ctx->safety - 0.02);
                    // the largest displacement since the build is both a fresh sample of the rate and the exact
                    // test of whether the outer rows can still serve a prune step at the drifted positions
                    double d0 = measure_disp0(pos_m);
                    double sample = d0 / (double)ctx->steps_since_build;
                    if (!ctx->rate_known)
                        ctx->d1_rate = sample;
                    else if (sample > ctx->d1_rate)
                        ctx->d1_rate = 0.5 * (ctx->d1_rate + sample);
                    ctx->rate_known = true;
                    // (a prune this late would buy only a few steps: rebuild unless a full segment still fits)
                    // (the rows a prune would write have the full inner skin; the outer rows what md_scale_cell left them)
                    if (m_was_prune || !(d0 + 0.5 * ctx->inner_skin <= 0.5 * skin_eff(ctx))) {
                        if (fused)
                            fused_rebuild();
                        else
                            rebuild(ctx);
                        rebuilt = true;
                    } else {
                        ctx->inner_valid = false;
                        rebuilt = false;
                    }
                }
                if (!rebuilt) {
                    // a prune step follows: consume the recorded violation, and redo the ghost refresh that
                    // was skipped along with the step's force half
                    k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
                    launch_ghost_update(ctx, -1);
                }
                if (was_fused) {
                    // the whole of step m again, from the state of step m-1 (a fused build happens at the step
                    // boundary: the rows are one step old when step m uses them)
                    step_part(m);
                    if (rebuilt) ctx->steps_since_build = 1;
                } else {
                    force_part(m);
                }
                ctx->steps_since_prune = 1;
                s = m + 1;
            } else {
                ctx->steps_since_build += win_end - s;
                s = win_end;
                if (pruning) {
                    if (!ctx->rate_known) {
                        ctx->d1_rate = measure_disp0() / (double)ctx->steps_since_build;
                        ctx->rate_known = true;
                    } else {
                        // d1 belongs to the window's last prune step
                        int64_t b_last = ctx->steps_since_build - (win_end - 1 - last_prune) - 1;
                        if (last_prune >= 0 && b_last > 0)
                            ctx->d1_rate = 0.7 * ctx->d1_rate + 0.3 * (d1 / (double)b_last);
                        ctx->safety = std::min(0.99, ctx->safety + 0.002);
                        if (s < (int)nsteps && ctx->steps_since_build >= R) {
                            if (fused)
                                fused_rebuild();
                            else
                                rebuild(ctx);
                        }
                    }
                } else if (s < (int)nsteps && ctx->steps_since_build >= ctx->target_interval) {
                    // scheduled rebuild just ahead of the expected violation; creep the interval up so that it
                    // tracks the true one from below
                    if (fused)
                        fused_rebuild();
                    else
                        rebuild(ctx);
                    ctx->target_interval += 1;
                }
            }
        }
    }
    if (ctx->dbg_stamps.p && ctx->use_tiles) {
        // MDHIP_STAMPS=1: phase cycle counts of the LAST fused launch, averaged over its waves
        std::vector<long long> hs((size_t)ctx->nblk * 4 * 8);
        HIPCHK(hipMemcpyAsync(hs.data(), ctx->dbg_stamps.p, hs.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double acc[6] = {0};
        long long t0 = LLONG_MAX, t1 = 0;
        for (size_t w = 0; w < (size_t)ctx->nblk * 4; ++w) {
            for (int i = 1; i <= 5; ++i) acc[i] += (double)(hs[w * 8 + i] - hs[w * 8 + i - 1]);
            t0 = std::min(t0, hs[w * 8]);
            t1 = std::max(t1, hs[w * 8 + 5]);
        }
        double nw = (double)ctx->nblk * 4;
        fprintf(stderr, "[mdhip] %s cycles/wave:", fused ? "step_tile" : "force_tile"); fprintf(stderr, " own %.0f stage %.0f barrier %.0f loop %.0f epilogue %.0f | kernel span %lld\n",
                acc[1] / nw, acc[2] / nw, acc[3] / nw, acc[4] / nw, acc[5] / nw, t1 - t0);
    }
    if (fused) {
        // records -> state arrays, with the last step's pending rescale applied (src/thermostat.jl:43-45)
        fused_leave(ctx, true);
        fscope.done = true;
        if (nvt) k_set_scale<<<1, 1, 0, st>>>(ctx->scal.p, 1.0);
    } else if (nvt) {
        // apply the last step's pending rescale (src/thermostat.jl:43-45) so the state the
        // host can download is the reference's
        DevState sd = ctx->dev(ctx->cur);
        if (ctx->dim == 3)
            k_scale_v<3><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, ctx->scal.p, 1.0, 1);
        else
            k_scale_v<2><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, ctx->scal.p, 1.0, 1);
        k_set_scale<<<1, 1, 0, st>>>(ctx->scal.p, 1.0);
    }
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    if (want) {
        uwk[0] = h.U;
        uwk[1] = h.W;
        uwk[2] = h.K;
    }
    if (h.halo_overflow & 16) {
        // the LAST step's prune found an inner halo that does not fit: nothing ran on those rows; drop them
        ctx->allow_inner_halo = false;
        ctx->inner_valid = false;
        k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
        k_clear_halo_overflow<<<1, 1, 0, st>>>(ctx->scal.p);
        HIPCHK(hipStreamSynchronize(st));
    }
    debug_tile_halos(ctx);
    ctx->st_steps += nsteps;
    API_END
}

// fire_minimize!: src/minimize.jl:31-135 (kernels and scheme: md_kernels.hpp, "FIRE relaxation")
int md_fire_minimize(md_ctx *ctx, int64_t max_steps, double tol, double dt_initial, double dt_max, double alpha0,
                     double f_inc, double f_dec, int nmin, int64_t *steps, int *converged, double *energy,
                     double *f_rms)
{
    API_BEGIN
    require_state(ctx, "md_fire_minimize");
    if (ctx->dom.on) throw HipError("md_fire_minimize: not available on a slab-decomposition handle");
    if (max_steps < 0 || max_steps > 0x3ffffff0) throw HipError("md_fire_minimize: bad max_steps");
    if (!(dt_initial > 0.0) || !(dt_max >= dt_initial)) throw HipError("md_fire_minimize: need 0 < dt_initial <= dt_max");
    hipStream_t st = ctx->stream;
    const size_t nd = (size_t)ctx->n * ctx->dim;
    // FIRE's velocities are internal and start at zero (src/minimize.jl:57): park the MD velocities on the host
    std::vector<double> vsave(nd), zeros(nd, 0.0);
    if (md_download(ctx, nullptr, vsave.data(), nullptr, nullptr) != 0) return 1;
    if (md_upload(ctx, nullptr, zeros.data(), nullptr, nullptr, nullptr) != 0) return 1;
    ctx->list_valid = false;
    FireState hf{};
    hf.dt = dt_initial;
    hf.alpha = alpha0;
    hf.dt_initial = dt_initial;
    hf.dt_max = dt_max;
    hf.alpha0 = alpha0;
    hf.f_inc = f_inc;
    hf.f_dec = f_dec;
    hf.tol = tol;
    hf.ndof = ctx->dim * ((double)ctx->n_global - 1.0);
    hf.nmin = nmin;
    hf.conv_step = -1;
    hf.mix_keep = 1.0;
    ctx->fire_state.ensure(1);
    HIPCHK(hipMemcpyAsync(ctx->fire_state.p, &hf, sizeof hf, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    auto eval = [&](int t, bool drift) {
        // (rows: the outer ones -- KICK = false never prunes, and the rebuild below left no inner rows)
        launch_force(ctx, true, false, 0.0, t);
        DevState s = ctx->dev(ctx->cur);
        int nb = ctx->nblk, n = (int)ctx->n;
        ctx->fire_part.ensure((size_t)3 * nb);
        if (ctx->dim == 3)
            k_fire_a<3><<<nb, MD_BLOCK, 0, st>>>(n, s, ctx->fire_state.p, ctx->fire_part.p, nb, ctx->scal.p, t);
        else
            k_fire_a<2><<<nb, MD_BLOCK, 0, st>>>(n, s, ctx->fire_state.p, ctx->fire_part.p, nb, ctx->scal.p, t);
        k_fire_reduce<<<1, 1024, 0, st>>>(nb, ctx->fire_part.p, nb, ctx->partials.p, ctx->fire_state.p, ctx->scal.p, t);
        if (!drift) return;
        if (ctx->dim == 3)
            k_fire_b<3><<<nb, MD_BLOCK, 0, st>>>(n, s, ctx->fire_state.p, 0.5 * ctx->skin, ctx->scal.p, t);
        else
            k_fire_b<2><<<nb, MD_BLOCK, 0, st>>>(n, s, ctx->fire_state.p, 0.5 * ctx->skin, ctx->scal.p, t);
        // ghost copies (rows without tiles, or 2^26 slots and more) follow their owners, as after md_run's drift
        launch_ghost_update(ctx, t);
    };
    auto read_fire = [&]() {
        HIPCHK(hipMemcpyAsync(&hf, ctx->fire_state.p, sizeof hf, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    };
    int64_t s = 0;
    bool conv = false;
    while (s < max_steps && !conv) {
        if (!ctx->list_valid) rebuild(ctx); // (wraps the positions, resets the violation word)
        int64_t chunk_end = std::min<int64_t>(max_steps, s + 32);
        for (int64_t t = s; t < chunk_end; ++t) eval((int)t, true);
        HIPCHK(hipGetLastError());
        Scalars h = read_scalars(ctx);
        read_fire();
        if (hf.converged) {
            conv = true;
            s = (int64_t)hf.conv_step + 1;
            k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
            break;
        }
        if (h.first_viol <= chunk_end) {
            // the drift of step first_viol-1 moved some particle skin/2 from its build position: the rows
            // must be rebuilt before that step's successor evaluates forces (kernels after it skipped)
            s = h.first_viol;
            ctx->list_valid = false;
            ctx->st_viol++;
        } else {
            s = chunk_end;
        }
    }
    if (!conv) {
        // src/minimize.jl:126-129: the closing force evaluation of a run that did not converge
        if (!ctx->list_valid) rebuild(ctx);
        double tol_keep = hf.tol;
        eval(-1, false);
        read_fire();
        (void)tol_keep;
        hf.converged = 0; // (the closing evaluation is not a convergence test)
        k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
    }
    if (md_upload(ctx, nullptr, vsave.data(), nullptr, nullptr, nullptr) != 0) return 1;
    ctx->list_valid = false; // (this loop kept none of the step loop's bookkeeping: the next md_run starts from a build)
    if (steps) *steps = s;
    if (converged) *converged = conv ? 1 : 0;
    if (energy) *energy = hf.energy;
    if (f_rms) *f_rms = hf.f_rms;
    API_END
}

// Brownian dynamics: the step loop of src/simulation.jl:181-308 (forces at x, then the Euler-Maruyama move of
// src/integrate.jl:66-82), device resident; noise from Philox keyed by (seed; particle id, first_step + s).
int md_run_brownian(md_ctx *ctx, int64_t nsteps, double dt, double ktemp, uint64_t seed, int64_t first_step,
                    int64_t virial_every, double *out)
{
    API_BEGIN
    require_state(ctx, "md_run_brownian");
    if (ctx->dom.on) throw HipError("md_run_brownian: not available on a slab-decomposition handle");
    if (nsteps < 0 || nsteps > 0x3ffffff0) throw HipError("md_run_brownian: bad nsteps");
    if (!(dt > 0.0) || !(ktemp > 0.0)) throw HipError("md_run_brownian: need dt > 0 and kT > 0");
    if (nsteps == 0) {
        // no force evaluation ran: nothing to report (the scalars still hold an earlier call's U / W) and no state to touch
        if (out) out[0] = out[1] = out[2] = out[3] = 0.0;
        return 0;
    }
    if (virial_every < 1) virial_every = 10;
    hipStream_t st = ctx->stream;
    ctx->brown_acc.ensure(2);
    HIPCHK(hipMemsetAsync(ctx->brown_acc.p, 0, 2 * sizeof(double), st));
    const double sigma = std::sqrt(2.0 * dt);
    ctx->list_valid = false; // (rows without inner pruning for this loop; positions may have been uploaded)
    int64_t s = 0;
    while (s < nsteps) {
        if (!ctx->list_valid) rebuild(ctx);
        int64_t chunk_end = std::min<int64_t>(nsteps, s + 32);
        for (int64_t t = s; t < chunk_end; ++t) {
            int64_t g = first_step + t;
            bool sample = (g % virial_every) == 0;
            bool want = sample || t == nsteps - 1;
            launch_force(ctx, want, false, 0.0, (int)t);
            if (want)
                k_brownian_sums<<<1, 1024, 0, st>>>(ctx->nblk, ctx->partials.p, sample ? 1 : 0, ctx->brown_acc.p, ctx->scal.p,
                                                    (int)t);
            DevState sd = ctx->dev(ctx->cur);
            if (ctx->dim == 3)
                k_brownian_move<3><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, dt, ktemp, sigma, seed, g,
                                                                   0.5 * ctx->skin, ctx->scal.p, (int)t);
            else
                k_brownian_move<2><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, dt, ktemp, sigma, seed, g,
                                                                   0.5 * ctx->skin, ctx->scal.p, (int)t);
            launch_ghost_update(ctx, (int)t); // (ghost copies follow their owners, as after md_run's drift)
        }
        HIPCHK(hipGetLastError());
        Scalars h = read_scalars(ctx);
        if (h.first_viol <= chunk_end) {
            // the move of step first_viol-1 took some particle skin/2 from its build position: rebuild before the
            // next force evaluation (everything enqueued after that move skipped itself)
            s = h.first_viol;
            ctx->list_valid = false;
            if (s < nsteps) ctx->st_viol++;
        } else {
            s = chunk_end;
        }
    }
    k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
    Scalars h = read_scalars(ctx);
    double acc[2];
    HIPCHK(hipMemcpyAsync(acc, ctx->brown_acc.p, sizeof acc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out) {
        out[0] = h.U;
        out[1] = h.W;
        out[2] = acc[0];
        out[3] = acc[1];
    }
    ctx->list_valid = false; // (see md_fire_minimize)
    ctx->st_steps += nsteps;
    API_END
}

int md_kinetic(md_ctx *ctx, double *kinetic)
{
    API_BEGIN
    require_state(ctx, "md_kinetic");
    DevState s = ctx->dev(ctx->cur);
    if (ctx->dim == 3)
        k_ke_partials<3><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, ctx->partials.p);
    else
        k_ke_partials<2><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, ctx->partials.p);
    launch_finalize(ctx, false, false, 1.0, 0.0, -1);
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    if (kinetic) *kinetic = h.K;
    API_END
}

int md_scale_velocities(md_ctx *ctx, double sfac)
{
    API_BEGIN
    require_state(ctx, "md_scale_velocities");
    DevState s = ctx->dev(ctx->cur);
    if (ctx->nblk <= 0) {
        // (a slab that owns no particle)
    } else if (ctx->dim == 3)
        k_scale_v<3><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, ctx->scal.p, sfac, 0);
    else
        k_scale_v<2><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, s, ctx->scal.p, sfac, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    API_END
}

int md_profile(md_ctx *ctx, int enable)
{
    API_BEGIN
    prof_collect(ctx);
    ctx->prof = enable != 0;
    ctx->prof_stride = enable > 1 ? enable : 1;
    ctx->prof_seen[0] = ctx->prof_seen[1] = 0;
    if (enable) {
        ctx->prof_ms_acc = 0.0;
        ctx->prof_launch_acc = 0;
        ctx->prof_kd_ms_acc = 0.0;
        ctx->prof_kd_launch_acc = 0;
        ctx->prof_prune_acc = 0;
        ctx->prof_prune_ms_acc = 0.0;
        ctx->prof_rebuild_acc = 0;
        ctx->prof_rebuild_ms_acc = 0.0;
    }
    API_END
}

int md_get_stats(md_ctx *ctx, md_stats *out)
{
    API_BEGIN
    if (!out) throw HipError("md_get_stats: out is null");
    prof_collect(ctx);
    out->steps = ctx->st_steps;
    out->rebuilds = ctx->st_rebuilds;
    out->violations = ctx->st_viol;
    out->n_ghost = ctx->nghost;
    out->max_neighbors = ctx->maxn;
    out->avg_neighbors = 0.0;
    if (ctx->list_valid) {
        std::vector<int32_t> h((size_t)ctx->n);
        HIPCHK(hipMemcpyAsync(h.data(), ctx->nneigh.p, sizeof(int32_t) * ctx->n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        double sum = 0.0;
        for (int32_t v : h) sum += v;
        out->avg_neighbors = sum / (double)ctx->n;
    }
    out->prunes = ctx->st_prunes;
    out->max_halo = ctx->use_tiles ? ctx->hstride : 0;
    out->tiled = ctx->use_tiles ? 1 : 0;
    out->force_launches = ctx->prof_launch_acc;
    out->force_ms = ctx->prof_ms_acc;
    out->kickdrift_launches = ctx->prof_kd_launch_acc;
    out->kickdrift_ms = ctx->prof_kd_ms_acc;
    out->fused = ctx->last_run_fused ? 1 : 0;
    out->walked_outer = out->walked_inner = 0;
    if (ctx->list_valid) {
        const int64_t nw = (ctx->n + 63) / 64;
        std::vector<int32_t> h((size_t)nw);
        HIPCHK(hipMemcpyAsync(h.data(), ctx->nmax_tile.p, sizeof(int32_t) * nw, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int32_t v : h) out->walked_outer += 64 * (int64_t)v;
        if (ctx->inner_valid) {
            HIPCHK(hipMemcpyAsync(h.data(), ctx->nmax_tile_in.p, sizeof(int32_t) * nw, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            for (int32_t v : h) out->walked_inner += 64 * (int64_t)v;
        }
    }
    out->prune_launches_timed = ctx->prof_prune_acc;
    out->prune_ms = ctx->prof_prune_ms_acc;
    out->rebuilds_timed = ctx->prof_rebuild_acc;
    out->rebuild_ms = ctx->prof_rebuild_ms_acc;
    out->fused_build = (ctx->list_valid && ctx->use_tiles && !ctx->have_nlist32) ? 1 : 0;
    out->own_first = ctx->own_first_staged ? 1 : 0;
    API_END
}


// ------------------------------------------------------------------------------------------
// Slab decomposition entry points (see include/mdhip.h).  The caller (one process per GPU)
// moves the packed buffers between ranks; everything else happens on the device.
// ------------------------------------------------------------------------------------------
namespace {
void dom_require(md_ctx *c)
{
    if (!c->dom.on) throw HipError("this handle was not created with md_create_domain");
}
DomCounters dom_read_counters(md_ctx *c)
{
    DomCounters h;
    HIPCHK(hipMemcpyAsync(&h, c->dom.counters.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.error & 1) throw HipError("a particle moved by more than one slab between list builds");
    if (h.error & 2) throw HipError("slab exchange buffer overflow (raise n_cap)");
    return h;
}
} // namespace

int md_dom_set_uniform(md_ctx *ctx, int uniform, double sigma)
{
    API_BEGIN
    dom_require(ctx);
    ctx->uniform_sigma = uniform != 0;
    ctx->sigma_u = sigma;
    configure_potential(ctx);
    ctx->list_valid = false;
    API_END
}

int md_dom_upload(md_ctx *ctx, int64_t n_own, const int32_t *ids, const double *x, const double *v, const double *f,
                  const int32_t *images, const double *diameters)
{
    API_BEGIN
    if (x && v && f) ctx->state_invalid = false; // (a complete new state)
    dom_require(ctx);
    if (n_own < 0 || n_own > ctx->ncap) throw HipError("md_dom_upload: n_own exceeds the handle's capacity");
    if (n_own > 0 && (!ids || !x)) throw HipError("md_dom_upload: ids and x are required");
    size_t nd = (size_t)n_own * ctx->dim;
    hipStream_t st = ctx->stream;
    DBuf<int32_t> d_ids;
    d_ids.alloc(n_own + 1);
    ctx->io_x.ensure(nd + 1);
    ctx->io_v.ensure(nd + 1);
    ctx->io_f.ensure(nd + 1);
    ctx->io_i.ensure(nd + 1);
    ctx->io_d.ensure(n_own + 1);
    if (n_own > 0) {
        HIPCHK(hipMemcpyAsync(d_ids.p, ids, n_own * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->io_x.p, x, nd * sizeof(double), hipMemcpyHostToDevice, st));
        if (v) HIPCHK(hipMemcpyAsync(ctx->io_v.p, v, nd * sizeof(double), hipMemcpyHostToDevice, st));
        if (f) HIPCHK(hipMemcpyAsync(ctx->io_f.p, f, nd * sizeof(double), hipMemcpyHostToDevice, st));
        if (images) HIPCHK(hipMemcpyAsync(ctx->io_i.p, images, nd * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (diameters) HIPCHK(hipMemcpyAsync(ctx->io_d.p, diameters, n_own * sizeof(double), hipMemcpyHostToDevice, st));
        DevState s = ctx->dev(ctx->cur);
        int nb = nblocks(n_own);
        if (ctx->dim == 3)
            k_import_local<3><<<nb, MD_BLOCK, 0, st>>>((int)n_own, s, d_ids.p, ctx->io_x.p, v ? ctx->io_v.p : nullptr,
                                                       f ? ctx->io_f.p : nullptr, images ? ctx->io_i.p : nullptr,
                                                       diameters ? ctx->io_d.p : nullptr);
        else
            k_import_local<2><<<nb, MD_BLOCK, 0, st>>>((int)n_own, s, d_ids.p, ctx->io_x.p, v ? ctx->io_v.p : nullptr,
                                                       f ? ctx->io_f.p : nullptr, images ? ctx->io_i.p : nullptr,
                                                       diameters ? ctx->io_d.p : nullptr);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));
    ctx->n = n_own;
    ctx->nblk = nblocks(n_own);
    ctx->src_count = n_own;
    ctx->list_valid = false;
    API_END
}

int md_dom_download(md_ctx *ctx, int64_t cap, int64_t *n_own, int32_t *ids, double *x, double *v, double *f,
                    int32_t *images)
{
    API_BEGIN
    require_state(ctx, "md_dom_download");
    dom_require(ctx);
    if (n_own) *n_own = ctx->n;
    if (cap < ctx->n) throw HipError("md_dom_download: output capacity is smaller than the owned count");
    int64_t n = ctx->n;
    if (n == 0) return 0;
    size_t nd = (size_t)n * ctx->dim;
    hipStream_t st = ctx->stream;
    DBuf<int32_t> d_ids;
    d_ids.alloc(n);
    ctx->io_x.ensure(nd);
    ctx->io_v.ensure(nd);
    ctx->io_f.ensure(nd);
    ctx->io_i.ensure(nd);
    DevState s = ctx->dev(ctx->cur);
    if (ctx->dim == 3)
        k_export_local<3><<<nblocks(n), MD_BLOCK, 0, st>>>((int)n, s, ctx->grid, d_ids.p, ctx->io_x.p, ctx->io_v.p,
                                                           ctx->io_f.p, ctx->io_i.p);
    else
        k_export_local<2><<<nblocks(n), MD_BLOCK, 0, st>>>((int)n, s, ctx->grid, d_ids.p, ctx->io_x.p, ctx->io_v.p,
                                                           ctx->io_f.p, ctx->io_i.p);
    HIPCHK(hipGetLastError());
    if (ids) HIPCHK(hipMemcpyAsync(ids, d_ids.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (x) HIPCHK(hipMemcpyAsync(x, ctx->io_x.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (v) HIPCHK(hipMemcpyAsync(v, ctx->io_v.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (f) HIPCHK(hipMemcpyAsync(f, ctx->io_f.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (images) HIPCHK(hipMemcpyAsync(images, ctx->io_i.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

// step 1 of a list build: wrap, decide ownership, pack the leavers.  nsend[2] = records for the
// left / right neighbour (MD_MIG_REC doubles each) now sitting in the send buffers.
int md_dom_migrate_pack(md_ctx *ctx, int64_t *nsend)
{
    API_BEGIN
    dom_require(ctx);
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    d.n_old = ctx->n;
    d.n_arr = 0;
    d.n_xh = 0;
    HIPCHK(hipMemsetAsync(d.counters.p, 0, 8 * sizeof(int32_t), st));
    int cap_rec = (int)(d.sbuf[0].n / MD_MIG_REC);
    double inv_w = (double)d.nranks / ctx->L[0];
    DevState s = ctx->dev(ctx->cur);
    if (d.n_old > 0) {
        if (ctx->dim == 3)
            k_dom_classify<3><<<nblocks(d.n_old), MD_BLOCK, 0, st>>>((int)d.n_old, s, ctx->grid, d.xlo, d.xhi, inv_w,
                                                                     d.rank, d.nranks, d.alive.p, d.sbuf[0].p,
                                                                     d.sbuf[1].p, cap_rec, (DomCounters *)d.counters.p);
        else
            k_dom_classify<2><<<nblocks(d.n_old), MD_BLOCK, 0, st>>>((int)d.n_old, s, ctx->grid, d.xlo, d.xhi, inv_w,
                                                                     d.rank, d.nranks, d.alive.p, d.sbuf[0].p,
                                                                     d.sbuf[1].p, cap_rec, (DomCounters *)d.counters.p);
        HIPCHK(hipGetLastError());
    }
    DomCounters h = dom_read_counters(ctx);
    d.nsend_mig[0] = h.mig[0];
    d.nsend_mig[1] = h.mig[1];
    if (nsend) {
        nsend[0] = h.mig[0];
        nsend[1] = h.mig[1];
    }
    ctx->list_valid = false;
    API_END
}

// raw access to the exchange buffers: side 0 = left neighbour, 1 = right neighbour.
int md_dom_set_step_buffers(md_ctx *ctx, void *send_left, void *send_right, void *recv_left, void *recv_right,
                            int64_t capacity_doubles)
{
    API_BEGIN
    dom_require(ctx);
    ctx->dom.ext_send[0] = (double *)send_left;
    ctx->dom.ext_send[1] = (double *)send_right;
    ctx->dom.ext_recv[0] = (double *)recv_left;
    ctx->dom.ext_recv[1] = (double *)recv_right;
    ctx->dom.ext_cap = (send_left && send_right && recv_left && recv_right) ? capacity_doubles : 0;
    API_END
}

int md_dom_get_sendbuf(md_ctx *ctx, int side, int64_t ndoubles, void *dst, int dst_is_device)
{
    API_BEGIN
    dom_require(ctx);
    if (side < 0 || side > 1 || ndoubles < 0 || (size_t)ndoubles > ctx->dom.sbuf[side].n)
        throw HipError("md_dom_get_sendbuf: bad arguments");
    if (ndoubles > 0) {
        HIPCHK(hipMemcpyAsync(dst, ctx->dom.sbuf[side].p, ndoubles * sizeof(double),
                              dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    API_END
}

int md_dom_put_recvbuf(md_ctx *ctx, int side, int64_t ndoubles, const void *src, int src_is_device)
{
    API_BEGIN
    dom_require(ctx);
    if (side < 0 || side > 1 || ndoubles < 0 || (size_t)ndoubles > ctx->dom.rbuf[side].n)
        throw HipError("md_dom_put_recvbuf: message larger than the receive buffer (raise n_cap)");
    if (ndoubles > 0) {
        HIPCHK(hipMemcpyAsync(ctx->dom.rbuf[side].p, src, ndoubles * sizeof(double),
                              src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    API_END
}

// step 2: adopt the arrivals (nrecv[side] records in the receive buffers)
int md_dom_migrate_unpack(md_ctx *ctx, const int64_t *nrecv)
{
    API_BEGIN
    dom_require(ctx);
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    int64_t tot = nrecv[0] + nrecv[1];
    if (d.n_old + tot > ctx->ncap) throw HipError("owned-particle capacity exceeded on migration (raise n_cap)");
    ensure_capacity(ctx, d.n_old + tot + 1);
    if ((size_t)(d.n_old + tot + 2) > d.alive.n) throw HipError("source table exceeded (raise n_cap)");
    DevState s = ctx->dev(ctx->cur);
    int64_t base = d.n_old;
    for (int sd = 0; sd < 2; ++sd) {
        if (nrecv[sd] > 0) {
            if (ctx->dim == 3)
                k_dom_unpack_mig<3><<<nblocks(nrecv[sd]), MD_BLOCK, 0, st>>>((int)nrecv[sd], (int)base, d.rbuf[sd].p, s,
                                                                            d.alive.p);
            else
                k_dom_unpack_mig<2><<<nblocks(nrecv[sd]), MD_BLOCK, 0, st>>>((int)nrecv[sd], (int)base, d.rbuf[sd].p, s,
                                                                            d.alive.p);
            base += nrecv[sd];
        }
    }
    HIPCHK(hipGetLastError());
    d.n_arr = tot;
    ctx->src_count = d.n_old + tot;
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

// step 3: select and pack the particles within rc+skin of the slab faces (MD_HALO_REC doubles each)
int md_dom_halo_pack(md_ctx *ctx, int64_t *nsend)
{
    API_BEGIN
    dom_require(ctx);
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    int n_own_src = (int)(d.n_old + d.n_arr);
    int cap_rec = (int)std::min<size_t>(d.sbuf[0].n / MD_HALO_REC, d.hs_src[0].n);
    HIPCHK(hipMemsetAsync(d.counters.p, 0, 8 * sizeof(int32_t), st));
    double shift_l = (d.rank == 0) ? ctx->L[0] : 0.0;
    double shift_r = (d.rank == d.nranks - 1) ? -ctx->L[0] : 0.0;
    DevState s = ctx->dev(ctx->cur);
    if (n_own_src > 0)
        k_dom_select_halo<<<nblocks(n_own_src), MD_BLOCK, 0, st>>>(n_own_src, s, d.xlo, d.xhi, ctx->rl, shift_l, shift_r,
                                                                   d.alive.p, d.sbuf[0].p, d.sbuf[1].p, d.hs_src[0].p,
                                                                   d.hs_src[1].p, cap_rec, (DomCounters *)d.counters.p);
    HIPCHK(hipGetLastError());
    DomCounters h = dom_read_counters(ctx);
    d.nsend_halo[0] = h.halo[0];
    d.nsend_halo[1] = h.halo[1];
    if (nsend) {
        nsend[0] = h.halo[0];
        nsend[1] = h.halo[1];
    }
    API_END
}

// step 4: adopt the neighbours' halo records as x-halo sources
int md_dom_halo_unpack(md_ctx *ctx, const int64_t *nrecv)
{
    API_BEGIN
    dom_require(ctx);
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    int64_t n_own_src = d.n_old + d.n_arr;
    int64_t tot = nrecv[0] + nrecv[1];
    if ((size_t)tot > d.xh_slot.n) throw HipError("x-halo capacity exceeded (raise n_cap)");
    ctx->src_count = n_own_src;
    ensure_capacity(ctx, n_own_src + tot + 1);
    if ((size_t)(n_own_src + tot + 2) > d.alive.n) throw HipError("source table exceeded (raise n_cap)");
    DevState s = ctx->dev(ctx->cur);
    int64_t base = n_own_src;
    for (int sd = 0; sd < 2; ++sd) {
        if (nrecv[sd] > 0) {
            k_dom_unpack_halo<<<nblocks(nrecv[sd]), MD_BLOCK, 0, st>>>((int)nrecv[sd], (int)base, d.rbuf[sd].p, s,
                                                                      d.alive.p);
            base += nrecv[sd];
        }
        d.nrecv_halo[sd] = nrecv[sd];
    }
    HIPCHK(hipGetLastError());
    d.n_xh = tot;
    ctx->src_count = n_own_src + tot;
    HIPCHK(hipStreamSynchronize(st));
    API_END
}

// after a list build: which tiles touch the slab faces (md_domain.hpp, k_dom_tile_class)
static void dom_classify_tiles(md_ctx *ctx)
{
    auto &d = ctx->dom;
    d.n_tiles_b = d.n_tiles_i = 0;
    const char *ov = getenv("MDHIP_DOM_OVERLAP"); // (only the overlapped window uses the classes)
    if (!(ov && ov[0] == '1') || !ctx->use_tiles || !ctx->virtual_ghosts || ctx->n <= 0) return;
    hipStream_t st = ctx->stream;
    const int nb = ctx->nblk;
    d.tile_flag.ensure(nb);
    d.tiles_b.ensure(nb);
    d.tiles_i.ensure(nb);
    HIPCHK(hipMemsetAsync(d.tile_flag.p, 0, nb * sizeof(int32_t), st));
    k_dom_tile_class<<<nb, MD_BLOCK, 0, st>>>(nb, ctx->halo.p, ctx->hcap, ctx->halo_count.p, (int)ctx->n, d.tile_flag.p);
    for (int sd = 0; sd < 2; ++sd)
        if (d.nsend_halo[sd] > 0)
            k_dom_mark_send<<<nblocks(d.nsend_halo[sd]), MD_BLOCK, 0, st>>>((int)d.nsend_halo[sd], d.send_slot[sd].p, d.tile_flag.p);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> fl(nb), lb, li;
    HIPCHK(hipMemcpyAsync(fl.data(), d.tile_flag.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int b = 0; b < nb; ++b) (fl[b] ? lb : li).push_back(b);
    if (!lb.empty()) HIPCHK(hipMemcpyAsync(d.tiles_b.p, lb.data(), lb.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!li.empty()) HIPCHK(hipMemcpyAsync(d.tiles_i.p, li.data(), li.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // (the host vectors go out of scope)
    d.n_tiles_b = (int)lb.size();
    d.n_tiles_i = (int)li.size();
    if (getenv("MDHIP_DEBUG"))
        fprintf(stderr, "[mdhip] rank %d slab tiles: %d boundary, %d interior\n", d.rank, d.n_tiles_b, d.n_tiles_i);
}

// step 5: sort, ghosts, neighbour rows; fix the per-step halo slot tables
int md_dom_build(md_ctx *ctx)
{
    API_BEGIN
    dom_require(ctx);
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    int64_t n_own_src = d.n_old + d.n_arr;
    rebuild(ctx);
    for (int sd = 0; sd < 2; ++sd)
        if (d.nsend_halo[sd] > 0)
            k_dom_map_slots<<<nblocks(d.nsend_halo[sd]), MD_BLOCK, 0, st>>>((int)d.nsend_halo[sd], d.hs_src[sd].p, 0,
                                                                           ctx->newslot.p, d.send_slot[sd].p);
    if (d.n_xh > 0)
        k_dom_map_slots<<<nblocks(d.n_xh), MD_BLOCK, 0, st>>>((int)d.n_xh, nullptr, (int)n_own_src, ctx->newslot.p,
                                                              d.xh_slot.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    d.n_old = ctx->n;
    d.n_arr = 0;
    d.xhalo_pos_stale = false;
    dom_classify_tiles(ctx);
    API_END
}

// first half of a step: (pending rescale,) half-kick, drift, displacement check, and the halo
// coordinates packed for the neighbours (3 doubles per record, nsend_halo[side] records).
int md_dom_step_begin(md_ctx *ctx, double dt, int *violated)
{
    API_BEGIN
    dom_require(ctx);
    if (!ctx->list_valid) throw HipError("md_dom_step_begin: no valid neighbour list (run the build sequence first)");
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
    if (ctx->n > 0) launch_kickdrift(ctx, true, dt, true, 0);
    k_set_scale<<<1, 1, 0, st>>>(ctx->scal.p, 1.0);
    DevState s = ctx->dev(ctx->cur);
    double shift_l = (d.rank == 0) ? ctx->L[0] : 0.0;
    double shift_r = (d.rank == d.nranks - 1) ? -ctx->L[0] : 0.0;
    for (int sd = 0; sd < 2; ++sd)
        if (d.nsend_halo[sd] > 0)
            k_dom_pack_pos<<<nblocks(d.nsend_halo[sd]), MD_BLOCK, 0, st>>>((int)d.nsend_halo[sd], d.send_slot[sd].p,
                                                                          s.pos, sd ? shift_r : shift_l,
                                                                          (d.ext_cap >= 3 * d.nsend_halo[sd]) ? d.ext_send[sd]
                                                                                                              : d.sbuf[sd].p);
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    if (violated) *violated = (h.first_viol != MD_NO_VIOLATION) ? 1 : 0;
    API_END
}

// second half: adopt the neighbours' halo coordinates, refresh the self-image ghosts, forces,
// second half-kick.  uwk receives this rank's share {U, W, K}.
int md_dom_step_end(md_ctx *ctx, double dt, int want_uw, double *uwk)
{
    API_BEGIN
    dom_require(ctx);
    auto &d = ctx->dom;
    d.xhalo_pos_stale = false; // (the coordinates just received are unpacked below)
    hipStream_t st = ctx->stream;
    DevState s = ctx->dev(ctx->cur);
    int64_t off = 0;
    for (int sd = 0; sd < 2; ++sd) {
        if (d.nrecv_halo[sd] > 0)
            k_dom_unpack_pos<<<nblocks(d.nrecv_halo[sd]), MD_BLOCK, 0, st>>>((int)d.nrecv_halo[sd], d.xh_slot.p + off,
                                                                            (d.ext_cap >= 3 * d.nrecv_halo[sd])
                                                                                ? d.ext_recv[sd]
                                                                                : d.rbuf[sd].p,
                                                                            s.pos);
        off += d.nrecv_halo[sd];
    }
    launch_ghost_update(ctx, -1);
    if (ctx->n > 0) {
        launch_force(ctx, want_uw != 0, true, dt, -1);
        launch_finalize(ctx, want_uw != 0, false, 1.0, 0.0, -1);
    }
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    if (uwk) {
        uwk[0] = (ctx->n > 0 && want_uw) ? h.U : 0.0;
        uwk[1] = (ctx->n > 0 && want_uw) ? h.W : 0.0;
        uwk[2] = (ctx->n > 0) ? h.K : 0.0;
    }
    ctx->st_steps += 1;
    API_END
}

// the force half alone (after a build triggered by a displacement violation, and for
// md_compute_forces-like calls): neighbours' coordinates are the ones delivered at the build.
int md_dom_forces(md_ctx *ctx, double dt, int kick, int want_uw, double *uwk)
{
    API_BEGIN
    require_state(ctx, "md_dom_forces");
    dom_require(ctx);
    if (!ctx->list_valid) throw HipError("md_dom_forces: no valid neighbour list");
    if (ctx->dom.xhalo_pos_stale)
        throw HipError("md_dom_forces: the x-halo coordinates are as of the last list build (a fused step window refreshes "
                       "only the state records); call md_dom_rebuild / md_dom_build, or a classic step's exchange, first");
    if (ctx->n > 0) {
        launch_force(ctx, want_uw != 0, kick != 0, dt, -1);
        launch_finalize(ctx, want_uw != 0, false, 1.0, 0.0, -1);
    }
    if (kick) ctx->steps_since_prune += 1; // the force half of a step
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    if (uwk) {
        uwk[0] = (ctx->n > 0 && want_uw) ? h.U : 0.0;
        uwk[1] = (ctx->n > 0 && want_uw) ? h.W : 0.0;
        uwk[2] = (ctx->n > 0 && kick) ? h.K : 0.0;
    }
    API_END
}

// ---------------------------------------------------------------------------------------------
// Asynchronous slab stepping: none of these waits for the device.  The caller enqueues, per step,
//   md_dom_step_a -> all-reduce(MIN) of flag_dev  +  neighbour exchange of the step buffers
//   md_dom_step_b -> all-reduce(SUM) of kuw_dev   (NVT, or when the step reports U/W/K)
//   md_dom_step_c
// on the handle's stream (md_set_stream: the caller's stream, so that its RCCL calls are ordered with the
// kernels), a whole window of steps at a time.  A displacement violation on any rank at step m reaches
// every rank through the reduced flag before step m's force evaluation: all later kernels of the window
// skip themselves on every rank, exactly as on one GPU.  md_dom_async_end waits and reports m.
// ---------------------------------------------------------------------------------------------
int md_set_stream(md_ctx *ctx, void *stream)
{
    API_BEGIN
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->stream = stream ? (hipStream_t)stream : ctx->own_stream;
    API_END
}

int md_dom_async_begin(md_ctx *ctx, int64_t nsteps, double dt, int ensemble, double tau, double nf,
                       const double *ktemp, const double *r1, const double *r2, int64_t prune_interval, void *flag_dev,
                       void *kuw_dev)
{
    API_BEGIN
    dom_require(ctx);
    if (!ctx->list_valid) throw HipError("md_dom_async_begin: no valid neighbour list (run the build sequence first)");
    if (!flag_dev || !kuw_dev) throw HipError("md_dom_async_begin: flag and K/U/W device words are required");
    if (nsteps < 0 || nsteps > 0x3fffffff) throw HipError("md_dom_async_begin: bad nsteps");
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    d.flag_dev = (int32_t *)flag_dev;
    d.kuw_dev = (double *)kuw_dev;
    d.a_nvt = ensemble == MD_NVT;
    d.a_nf = nf;
    d.a_term1 = 0.0;
    d.w_nsteps = nsteps;
    d.w_b0 = ctx->steps_since_build;
    d.w_prune_interval = prune_interval;
    d.w_prune_steps.clear();
    d.w_scale_from_sums = false; // step 0 of a window takes the pending scale from sc->scale
    if (d.a_nvt) {
        if (!ktemp || !r1 || !r2) throw HipError("md_dom_async_begin: NVT needs ktemp, r1, r2");
        if (!(tau > 0.0) || !(nf > 0.0)) throw HipError("md_dom_async_begin: NVT needs tau > 0 and nf > 0");
        ctx->d_kt.ensure(nsteps);
        ctx->d_r1.ensure(nsteps);
        ctx->d_r2.ensure(nsteps);
        HIPCHK(hipMemcpyAsync(ctx->d_kt.p, ktemp, nsteps * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->d_r1.p, r1, nsteps * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->d_r2.p, r2, nsteps * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // the host arrays are borrowed for this call only
        d.a_term1 = std::exp(-(dt / tau));
    }
    if (!d.a_nvt) k_set_scale<<<1, 1, 0, st>>>(ctx->scal.p, 1.0);
    k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
    HIPCHK(hipGetLastError());
    API_END
}

// pending rescale, half-kick, drift, displacement check; halo coordinates packed; this rank's flag exported
int md_dom_step_a(md_ctx *ctx, double dt, int step)
{
    API_BEGIN
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    // inner rows: the schedule (identical on every rank) is the caller's prune interval
    if (ctx->prune_on && ctx->inner_valid && d.w_prune_interval > 0 && ctx->steps_since_prune >= d.w_prune_interval)
        ctx->inner_valid = false;
    if (ctx->prune_on && !ctx->inner_valid) d.w_prune_steps.push_back(step);
    BussiSrc bs{};
    if (d.a_nvt && d.w_scale_from_sums) {
        // the previous step's md_dom_step_c was skipped: its Bussi scale is formed here from the reduced sums
        bs.sums = d.kuw_dev;
        bs.kt = ctx->d_kt.p;
        bs.r1 = ctx->d_r1.p;
        bs.r2 = ctx->d_r2.p;
        bs.nf = d.a_nf;
        bs.term1 = d.a_term1;
        bs.idx = step - 1;
    }
    d.w_scale_from_sums = d.a_nvt; // until md_dom_step_c runs for this step
    if (ctx->n > 0) launch_kickdrift(ctx, true, dt, true, step, bs);
    DevState s = ctx->dev(ctx->cur);
    double shift_l = (d.rank == 0) ? ctx->L[0] : 0.0;
    double shift_r = (d.rank == d.nranks - 1) ? -ctx->L[0] : 0.0;
    double *out[2];
    for (int sd = 0; sd < 2; ++sd) out[sd] = (d.ext_cap >= 3 * d.nsend_halo[sd]) ? d.ext_send[sd] : d.sbuf[sd].p;
    int n0 = (int)d.nsend_halo[0], n1 = (int)d.nsend_halo[1];
    k_dom_pack_pos2<<<nblocks(std::max(n0 + n1, 1)), MD_BLOCK, 0, st>>>(n0, n1, d.send_slot[0].p, d.send_slot[1].p, s.pos,
                                                                        shift_l, shift_r, out[0], out[1], ctx->scal.p,
                                                                        d.flag_dev);
    HIPCHK(hipGetLastError());
    API_END
}

// reduced flag adopted; neighbours' halo coordinates adopted; self-image ghosts; forces + second half-kick;
// this rank's K (U, W) sums exported
int md_dom_step_b(md_ctx *ctx, double dt, int step, int want_uw)
{
    API_BEGIN
    auto &d = ctx->dom;
    d.xhalo_pos_stale = false; // (the coordinates just received are unpacked below)
    hipStream_t st = ctx->stream;
    DevState s = ctx->dev(ctx->cur);
    double *in[2];
    for (int sd = 0; sd < 2; ++sd) in[sd] = (d.ext_cap >= 3 * d.nrecv_halo[sd]) ? d.ext_recv[sd] : d.rbuf[sd].p;
    int n0 = (int)d.nrecv_halo[0], n1 = (int)d.nrecv_halo[1];
    k_dom_unpack_pos2<<<nblocks(std::max(n0 + n1, 1)), MD_BLOCK, 0, st>>>(n0, n1, d.xh_slot.p, in[0], in[1], s.pos,
                                                                          ctx->scal.p, d.flag_dev);
    launch_ghost_update(ctx, step); // (nothing to do with virtual ghosts)
    if (ctx->n > 0) launch_force(ctx, want_uw != 0, true, dt, step);
    k_dom_local_sums<<<1, 1024, 0, st>>>(ctx->n > 0 ? ctx->nblk : 0, ctx->partials.p, want_uw, d.kuw_dev, ctx->scal.p, step);
    HIPCHK(hipGetLastError());
    ctx->st_steps += 1;
    ctx->steps_since_prune += 1;
    API_END
}

// from the reduced sums: global K (U, W); Bussi scale of this step, applied by the next md_dom_step_a
int md_dom_step_c(md_ctx *ctx, int step, int want_uw)
{
    API_BEGIN
    auto &d = ctx->dom;
    k_dom_global_finalize<<<1, 1, 0, ctx->stream>>>(d.kuw_dev, want_uw, d.a_nvt ? 1 : 0, d.a_nf, d.a_term1, ctx->d_kt.p,
                                                    ctx->d_r1.p, ctx->d_r2.p, ctx->scal.p, step);
    d.w_scale_from_sums = false; // sc->scale now holds this step's scale
    HIPCHK(hipGetLastError());
    API_END
}

// waits for the window; first_viol = first step at which some rank's displacement check failed (or
// 0x7fffffff); uwk = global {U, W, K} of the last executed step that reported them
int md_dom_async_end(md_ctx *ctx, int apply_pending_scale, int32_t *first_viol, double *uwk, double *info)
{
    API_BEGIN
    dom_require(ctx);
    if (apply_pending_scale && ctx->dom.a_nvt && ctx->n > 0) {
        // the last step's rescale (src/thermostat.jl:43-45) is still pending: apply it so that the state the
        // host can download is the reference's.  Skipped by the kernel itself after a violation (the pending
        // scale was then already consumed by the violating step's drift).
        DevState sd = ctx->dev(ctx->cur);
        if (ctx->dim == 3)
            k_scale_v<3><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, sd, ctx->scal.p, 1.0, 2);
        else
            k_scale_v<2><<<ctx->nblk, MD_BLOCK, 0, ctx->stream>>>((int)ctx->n, sd, ctx->scal.p, 1.0, 2);
        k_set_scale_unless_violated<<<1, 1, 0, ctx->stream>>>(ctx->scal.p, 1.0);
    }
    Scalars h = read_scalars(ctx);
    if (first_viol) *first_viol = h.first_viol;
    if (uwk) {
        uwk[0] = h.U;
        uwk[1] = h.W;
        uwk[2] = h.K;
    }
    // bookkeeping + what the caller's planner needs
    auto &d = ctx->dom;
    int64_t fv = h.first_viol;
    int64_t done = fv < d.w_nsteps ? fv + 1 : d.w_nsteps; // steps whose drift was executed
    ctx->steps_since_build = d.w_b0 + done;
    bool was_prune = false;
    int last_prune = -1;
    for (int p : d.w_prune_steps) {
        if (p == fv) was_prune = true;
        if (p < fv && p < d.w_nsteps) last_prune = p;
    }
    if (info) {
        double d12;
        unsigned long long bits = h.d1max2_bits;
        memcpy(&d12, &bits, sizeof d12);
        info[0] = was_prune ? 1.0 : 0.0;
        info[1] = std::sqrt(d12);
        info[2] = last_prune >= 0 ? (double)(d.w_b0 + last_prune + 1) : -1.0;
        info[3] = ctx->prune_on ? 1.0 : 0.0;
        info[4] = ctx->skin;
        info[5] = ctx->prune_on ? ctx->inner_skin : 0.0;
    }
    API_END
}

// ---------------------------------------------------------------------------------------------
// Native transport: the window loop of the asynchronous scheme above entirely inside the library, the
// collectives issued by the library itself (RCCL over xGMI) on the handle's stream -- no host work and no
// stream hand-over between a step's kernels and its three small collectives.
// ---------------------------------------------------------------------------------------------
int md_dom_comm_unique_id(const char *rccl_path, void *id128)
{
    try {
        if (!id128) throw std::runtime_error("md_dom_comm_unique_id: null output");
        g_rccl.load(rccl_path);
        ncclUniqueId id;
        g_rccl.check(g_rccl.GetUniqueId(&id), "ncclGetUniqueId");
        memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
        return 0;
    } catch (const std::exception &e) {
        return fail(nullptr, e.what());
    }
}

static void dom_p2p_setup(md_ctx *ctx);

int md_dom_comm_init(md_ctx *ctx, const char *rccl_path, const void *id128)
{
    API_BEGIN
    dom_require(ctx);
    if (!id128) throw HipError("md_dom_comm_init: null unique id");
    auto &d = ctx->dom;
    g_rccl.load(rccl_path);
    if (d.comm) {
        (void)g_rccl.CommDestroy(d.comm);
        d.comm = nullptr;
    }
    ncclUniqueId id;
    memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    g_rccl.check(g_rccl.CommInitRank(&d.comm, d.nranks, id, d.rank), "ncclCommInitRank");
    d.own_flag.alloc(4);
    d.own_kuw.alloc(4);
    // self-test: the sum of (rank + 1) over the ranks, and the minimum of (rank + 7)
    hipStream_t st = ctx->stream;
    double hv[3] = {(double)(d.rank + 1), 1.0, 0.0};
    int32_t hf = d.rank + 7;
    HIPCHK(hipMemcpyAsync(d.own_kuw.p, hv, sizeof hv, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d.own_flag.p, &hf, sizeof hf, hipMemcpyHostToDevice, st));
    g_rccl.check(g_rccl.AllReduce(d.own_kuw.p, d.own_kuw.p, 3, ncclFloat64, ncclSum, d.comm, st), "ncclAllReduce");
    g_rccl.check(g_rccl.AllReduce(d.own_flag.p, d.own_flag.p, 1, ncclInt32, ncclMin, d.comm, st), "ncclAllReduce");
    HIPCHK(hipMemcpyAsync(hv, d.own_kuw.p, sizeof hv, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hf, d.own_flag.p, sizeof hf, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double want = 0.5 * d.nranks * (d.nranks + 1.0);
    if (hv[0] != want || hv[1] != (double)d.nranks || hf != 7)
        throw HipError("md_dom_comm_init: RCCL self-test returned wrong values");
    dom_p2p_setup(ctx);
    API_END
}

int md_dom_enable_pruning(md_ctx *ctx, int on)
{
    API_BEGIN
    dom_require(ctx);
    ctx->dom.prune_enabled = on != 0;
    ctx->list_valid = false;
    API_END
}

// this rank's largest displacement since the list build, max_i |x_i - x0_i| (exact; waits for the device)
int md_dom_max_disp0(md_ctx *ctx, double *d0)
{
    API_BEGIN
    dom_require(ctx);
    hipStream_t st = ctx->stream;
    k_reset_disp0<<<1, 1, 0, st>>>(ctx->scal.p);
    if (ctx->n > 0) {
        DevState sd = ctx->dev(ctx->cur);
        if (ctx->dim == 3)
            k_max_disp0<3><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, ctx->scal.p);
        else
            k_max_disp0<2><<<ctx->nblk, MD_BLOCK, 0, st>>>((int)ctx->n, sd, ctx->scal.p);
    }
    Scalars h = read_scalars(ctx);
    double d0sq;
    unsigned long long bits = h.max_disp2_bits;
    memcpy(&d0sq, &bits, sizeof d0sq);
    if (d0) *d0 = std::sqrt(d0sq);
    API_END
}

// the next force evaluation refreshes the inner rows (a prune step) -- after a violation of the inner rows'
// criterion that the outer rows survived
int md_dom_invalidate_inner(md_ctx *ctx)
{
    API_BEGIN
    dom_require(ctx);
    ctx->inner_valid = false;
    k_reset_viol<<<1, 1, 0, ctx->stream>>>(ctx->scal.p);
    API_END
}

// A failure on this rank between collectives would leave its peers blocked inside theirs: abort the communicator
// first so that they fail fast instead of hanging (the handle needs md_dom_comm_init again).
// ---- direct peer exchange: mailbox layout, set-up, tear-down (md_domain.hpp "direct peer exchange") -----------------
// mailbox of a rank:  [2 record flags | nranks sum flags] (one per 128-byte line)  [2 planes][nranks][4] sums
//                     [from-left, from-right][2 planes][6][cap] record words
static size_t p2p_round(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t p2p_off_rec_flag(int side) { return (size_t)side * 128; }
static size_t p2p_off_sum_flag(int r) { return (size_t)(2 + r) * 128; }
static size_t p2p_off_sums(int nranks, int plane, int r) { return p2p_round((size_t)(2 + nranks) * 128) + ((size_t)plane * nranks + r) * 32; }
static size_t p2p_off_recs(int nranks, int64_t cap, int side, int plane)
{
    return p2p_round(p2p_off_sums(nranks, 2, 0)) + (size_t)(side * 2 + plane) * 6 * (size_t)cap * sizeof(double);
}
static size_t p2p_bytes(int nranks, int64_t cap) { return p2p_off_recs(nranks, cap, 2, 0); }

static void dom_p2p_teardown(md_ctx *c)
{
    auto &q = c->dom.p2p;
    for (int r = 0; r < MD_P2P_MAXR; ++r) {
        if (q.opened[r] && q.peer[r]) (void)hipIpcCloseMemHandle(q.peer[r]);
        q.opened[r] = false;
        q.peer[r] = nullptr;
    }
    if (q.mail) (void)hipFree(q.mail);
    if (q.done) (void)hipFree(q.done);
    q.mail = nullptr;
    q.done = nullptr;
    q.on = false;
    q.window = false;
    q.seq = 0;
}

// a failing rank tells its peers: every flag this rank owns in their mailboxes takes the poison value, so that a peer
// waiting for this rank stops at once (comm_error 2) instead of running into its timeout.  Never throws.
static void dom_p2p_poison(md_ctx *c)
{
    auto &d = c->dom;
    auto &q = d.p2p;
    if (!q.on) return;
    const unsigned long long poison = MD_P2P_POISON;
    const int left = (d.rank + d.nranks - 1) % d.nranks, right = (d.rank + 1) % d.nranks;
    for (int r = 0; r < d.nranks; ++r)
        if (q.peer[r]) (void)hipMemcpy(q.peer[r] + p2p_off_sum_flag(d.rank), &poison, sizeof poison, hipMemcpyHostToDevice);
    if (q.peer[left]) (void)hipMemcpy(q.peer[left] + p2p_off_rec_flag(1), &poison, sizeof poison, hipMemcpyHostToDevice);
    if (q.peer[right]) (void)hipMemcpy(q.peer[right] + p2p_off_rec_flag(0), &poison, sizeof poison, hipMemcpyHostToDevice);
    q.on = false; // (the sequence numbers are out of step from here on: md_dom_comm_init builds a fresh set)
}

static P2pPut dom_p2p_put_args(md_ctx *c, unsigned long long seq)
{
    auto &d = c->dom;
    auto &q = d.p2p;
    P2pPut a{};
    a.on = 1;
    a.nranks = d.nranks;
    a.seq = seq;
    const int plane = (int)(seq & 1ull);
    for (int r = 0; r < d.nranks; ++r) {
        a.sum_slot[r] = (double *)(q.peer[r] + p2p_off_sums(d.nranks, plane, d.rank));
        a.sum_flag[r] = (unsigned long long *)(q.peer[r] + p2p_off_sum_flag(d.rank));
    }
    const int left = (d.rank + d.nranks - 1) % d.nranks, right = (d.rank + 1) % d.nranks;
    a.rec_flag[0] = (unsigned long long *)(q.peer[left] + p2p_off_rec_flag(1));  // the left neighbour's "from my right"
    a.rec_flag[1] = (unsigned long long *)(q.peer[right] + p2p_off_rec_flag(0)); // the right neighbour's "from my left"
    a.done = q.done;
    return a;
}
static P2pGet dom_p2p_get_args(md_ctx *c, unsigned long long seq, long long timeout)
{
    auto &d = c->dom;
    auto &q = d.p2p;
    P2pGet a{};
    a.on = 1;
    a.nranks = d.nranks;
    a.seq = seq;
    a.sum_slot = (const double *)(q.mail + p2p_off_sums(d.nranks, (int)(seq & 1ull), 0));
    a.sum_flag = (const unsigned long long *)(q.mail + p2p_off_sum_flag(0));
    a.rec_flag[0] = (const unsigned long long *)(q.mail + p2p_off_rec_flag(0));
    a.rec_flag[1] = (const unsigned long long *)(q.mail + p2p_off_rec_flag(1));
    a.timeout = timeout;
    return a;
}
// where this rank's records for a neighbour go (side 0: to the left neighbour, 1: to the right), and where its own arrive
static double *dom_p2p_send_plane(md_ctx *c, int side, unsigned long long seq)
{
    auto &d = c->dom;
    const int peer = side == 0 ? (d.rank + d.nranks - 1) % d.nranks : (d.rank + 1) % d.nranks;
    // (what goes to the left neighbour is what it receives "from the right")
    return (double *)(d.p2p.peer[peer] + p2p_off_recs(d.nranks, d.p2p.peer_cap[peer], side == 0 ? 1 : 0, (int)(seq & 1ull)));
}
static double *dom_p2p_recv_plane(md_ctx *c, int side, unsigned long long seq)
{
    auto &d = c->dom;
    return (double *)(d.p2p.mail + p2p_off_recs(d.nranks, d.p2p.cap, side, (int)(seq & 1ull)));
}

// Collective (called from md_dom_comm_init, after the communicator's own self-test).  Every step that can fail on some
// rank only lowers `ok`; the ranks agree on the outcome (all-reduce MIN) and either all use the direct exchange or none.
static void dom_p2p_setup(md_ctx *ctx)
{
    auto &d = ctx->dom;
    auto &q = d.p2p;
    dom_p2p_teardown(ctx);
    hipStream_t st = ctx->stream;
    int ok = 1;
    const char *why = "";
    if (const char *e = getenv("MDHIP_DOM_P2P"))
        if (e[0] == '0') {
            ok = 0;
            why = "MDHIP_DOM_P2P=0";
        }
    if (d.nranks > MD_P2P_MAXR) return; // (every rank sees the same count: nothing to agree on)
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    const int R = d.nranks;
    q.cap = ctx->ncap;
    hipIpcMemHandle_t mine;
    memset(&mine, 0, sizeof mine);
    if (ok) {
        const size_t bytes = p2p_bytes(R, q.cap);
        if (hipExtMallocWithFlags((void **)&q.mail, bytes, hipDeviceMallocFinegrained) != hipSuccess || !q.mail) {
            (void)hipGetLastError();
            q.mail = nullptr;
            ok = 0;
            why = "no fine-grained device memory";
        } else {
            HIPCHK(hipMemsetAsync(q.mail, 0, p2p_off_recs(R, q.cap, 0, 0), st)); // flags and sums
            HIPCHK(hipMalloc((void **)&q.done, sizeof(unsigned)));
            HIPCHK(hipMemsetAsync(q.done, 0, sizeof(unsigned), st));
            HIPCHK(hipStreamSynchronize(st));
            if (R > 1 && hipIpcGetMemHandle(&mine, q.mail) != hipSuccess) {
                (void)hipGetLastError();
                ok = 0;
                why = "hipIpcGetMemHandle failed";
            }
        }
    }
    // handles and capacities travel through the communicator: rank r's 64 bytes as 64 doubles, everyone else adds zeros
    DBuf<double> tmp;
    tmp.alloc(64);
    std::vector<hipIpcMemHandle_t> handles(R);
    std::vector<double> caps(R, 0.0);
    if (R > 1) {
        for (int r = 0; r < R; ++r) {
            double h[64];
            for (int i = 0; i < 64; ++i) h[i] = (r == d.rank && ok) ? (double)((const unsigned char *)&mine)[i] : 0.0;
            HIPCHK(hipMemcpyAsync(tmp.p, h, sizeof h, hipMemcpyHostToDevice, st));
            g_rccl.check(g_rccl.AllReduce(tmp.p, tmp.p, 64, ncclFloat64, ncclSum, d.comm, st), "ncclAllReduce(mailbox handle)");
            HIPCHK(hipMemcpyAsync(h, tmp.p, sizeof h, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (int i = 0; i < 64; ++i) ((unsigned char *)&handles[r])[i] = (unsigned char)h[i];
        }
        double h[64] = {};
        h[d.rank] = ok ? (double)q.cap : 0.0;
        HIPCHK(hipMemcpyAsync(tmp.p, h, sizeof h, hipMemcpyHostToDevice, st));
        g_rccl.check(g_rccl.AllReduce(tmp.p, tmp.p, R, ncclFloat64, ncclSum, d.comm, st), "ncclAllReduce(mailbox capacity)");
        HIPCHK(hipMemcpyAsync(h, tmp.p, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int r = 0; r < R; ++r) {
            caps[r] = h[r];
            if (!(h[r] > 0.0) && ok) {
                ok = 0;
                why = "a peer has no mailbox";
            }
        }
    } else {
        caps[0] = (double)q.cap;
    }
    if (ok) {
        for (int r = 0; r < R; ++r) {
            q.peer_cap[r] = (int64_t)caps[r];
            if (r == d.rank) {
                q.peer[r] = q.mail;
                continue;
            }
            void *pp = nullptr;
            if (hipIpcOpenMemHandle(&pp, handles[r], hipIpcMemLazyEnablePeerAccess) != hipSuccess || !pp) {
                (void)hipGetLastError();
                ok = 0;
                why = "hipIpcOpenMemHandle failed (no peer access to that device?)";
                break;
            }
            q.peer[r] = (char *)pp;
            q.opened[r] = true;
        }
    }
    // rehearsal: one exchange without records, known sums, short timeout.  (Every rank runs it or none: a rank that
    // cannot would leave the others waiting, so the decision so far is agreed on first.)
    auto agree = [&](int v) {
        int32_t hf = v;
        HIPCHK(hipMemcpyAsync(d.own_flag.p, &hf, sizeof hf, hipMemcpyHostToDevice, st));
        g_rccl.check(g_rccl.AllReduce(d.own_flag.p, d.own_flag.p, 1, ncclInt32, ncclMin, d.comm, st), "ncclAllReduce(direct exchange)");
        HIPCHK(hipMemcpyAsync(&hf, d.own_flag.p, sizeof hf, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return (int)hf;
    };
    int all = agree(ok);
    if (all) {
        q.on = true;
        q.seq = 1;
        k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
        // (what this rank sends left arrives "from the right" at its left neighbour: tag 1000 (sender + 1) + side of arrival)
        const int left = (d.rank + R - 1) % R, right = (d.rank + 1) % R;
        k_p2p_hello_put<<<2, MD_BLOCK, 0, st>>>(dom_p2p_put_args(ctx, q.seq), (double)(d.rank + 1), dom_p2p_send_plane(ctx, 0, q.seq),
                                                dom_p2p_send_plane(ctx, 1, q.seq), 1000.0 * (d.rank + 1) + 100.0,
                                                1000.0 * (d.rank + 1));
        k_p2p_hello_get<<<2, MD_BLOCK, 0, st>>>(dom_p2p_get_args(ctx, q.seq, 10ll * 100000000ll), ctx->scal.p, tmp.p,
                                                dom_p2p_recv_plane(ctx, 0, q.seq), dom_p2p_recv_plane(ctx, 1, q.seq),
                                                1000.0 * (left + 1), 1000.0 * (right + 1) + 100.0);
        double h[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(h, tmp.p, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h[2] != 0.0 || h[3] != 0.0 || h[0] != 0.5 * R * (R + 1.0) || h[1] != (double)R) {
            ok = 0;
            why = "the rehearsal exchange did not deliver";
        }
        k_reset_viol<<<1, 1, 0, st>>>(ctx->scal.p);
        all = agree(ok);
    }
    if (!all) {
        if (d.rank == 0 && !(getenv("MDHIP_DOM_P2P") && getenv("MDHIP_DOM_P2P")[0] == '0'))
            fprintf(stderr, "[mdhip] direct peer exchange not in use (%s); the slab step keeps its RCCL collectives\n",
                    ok ? "a peer could not set it up" : why);
        dom_p2p_teardown(ctx);
        return;
    }
    double tsec = 60.0;
    if (const char *e = getenv("MDHIP_P2P_TIMEOUT_S")) tsec = std::max(0.5, atof(e));
    q.timeout = (long long)(tsec * 1e8);
    if (getenv("MDHIP_DEBUG"))
        fprintf(stderr, "[mdhip] rank %d: direct peer exchange ready (%d ranks, %lld records per plane, %.1f MB mailbox)\n", d.rank, R,
                (long long)q.cap, 1e-6 * (double)p2p_bytes(R, q.cap));
}

struct DomAbortGuard {
    md_ctx *c;
    bool armed = true;
    ~DomAbortGuard()
    {
        if (!armed) return;
        dom_p2p_poison(c);
        if (c->dom.comm && g_rccl.CommAbort) {
            (void)g_rccl.CommAbort(c->dom.comm);
            c->dom.comm = nullptr;
        }
    }
};

// Neighbour exchange of record sets whose sizes only the sender knows (migrants, halo records of a list build): the
// counts travel first, then the payloads straight from / into the library's exchange buffers, on the handle's stream.
// (issue order: see md_dom_run_window -- with one or two ranks both neighbours are the same peer)
static void dom_exchange_var(md_ctx *ctx, const int64_t *nsend, int rec, int64_t *nrecv)
{
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    const int left = (d.rank + d.nranks - 1) % d.nranks, right = (d.rank + 1) % d.nranks;
    d.cnt_dev.ensure(4);
    int64_t hc[4] = {nsend[0], nsend[1], 0, 0};
    HIPCHK(hipMemcpyAsync(d.cnt_dev.p, hc, 2 * sizeof(int64_t), hipMemcpyHostToDevice, st));
    g_rccl.check(g_rccl.GroupStart(), "ncclGroupStart");
    g_rccl.check(g_rccl.Send(d.cnt_dev.p + 0, 1, ncclInt64, left, d.comm, st), "ncclSend(count)");
    g_rccl.check(g_rccl.Send(d.cnt_dev.p + 1, 1, ncclInt64, right, d.comm, st), "ncclSend(count)");
    g_rccl.check(g_rccl.Recv(d.cnt_dev.p + 3, 1, ncclInt64, right, d.comm, st), "ncclRecv(count)");
    g_rccl.check(g_rccl.Recv(d.cnt_dev.p + 2, 1, ncclInt64, left, d.comm, st), "ncclRecv(count)");
    g_rccl.check(g_rccl.GroupEnd(), "ncclGroupEnd");
    HIPCHK(hipMemcpyAsync(hc + 2, d.cnt_dev.p + 2, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    nrecv[0] = hc[2]; // from the left neighbour
    nrecv[1] = hc[3]; // from the right neighbour
    for (int sd = 0; sd < 2; ++sd) {
        if (nrecv[sd] < 0 || (size_t)(nrecv[sd] * rec) > d.rbuf[sd].n)
            throw HipError("list build: a neighbour sends more records than the exchange buffers hold (raise n_cap)");
        if ((size_t)(nsend[sd] * rec) > d.sbuf[sd].n) throw HipError("list build: send buffer exceeded (raise n_cap)");
    }
    if (nsend[0] + nsend[1] + nrecv[0] + nrecv[1] == 0) return;
    g_rccl.check(g_rccl.GroupStart(), "ncclGroupStart");
    if (nsend[0] > 0) g_rccl.check(g_rccl.Send(d.sbuf[0].p, nsend[0] * rec, ncclFloat64, left, d.comm, st), "ncclSend");
    if (nsend[1] > 0) g_rccl.check(g_rccl.Send(d.sbuf[1].p, nsend[1] * rec, ncclFloat64, right, d.comm, st), "ncclSend");
    if (nrecv[1] > 0) g_rccl.check(g_rccl.Recv(d.rbuf[1].p, nrecv[1] * rec, ncclFloat64, right, d.comm, st), "ncclRecv");
    if (nrecv[0] > 0) g_rccl.check(g_rccl.Recv(d.rbuf[0].p, nrecv[0] * rec, ncclFloat64, left, d.comm, st), "ncclRecv");
    g_rccl.check(g_rccl.GroupEnd(), "ncclGroupEnd");
}

// MDHIP_DEBUG=1: the sizes of the tiles' halos (outer: staged by prune steps; inner: staged by ordinary steps)
static void debug_tile_halos(md_ctx *ctx)
{
    if (!getenv("MDHIP_DEBUG") || ctx->nblk <= 0 || !ctx->use_tiles) return;
    if (!ctx->inner_halo_live || ctx->halo_in_count.n < (size_t)ctx->nblk) {
        fprintf(stderr, "[mdhip] tile halos: no inner halo in use (allowed %d, inner rows %d valid %d)\n", (int)ctx->allow_inner_halo,
                (int)ctx->prune_on, (int)ctx->inner_valid);
        return;
    }
    std::vector<int32_t> hi(ctx->nblk), ho(ctx->nblk);
    HIPCHK(hipMemcpy(hi.data(), ctx->halo_in_count.p, ctx->nblk * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ho.data(), ctx->halo_count.p, ctx->nblk * sizeof(int32_t), hipMemcpyDeviceToHost));
    long long si = 0, so = 0;
    int mi = 0, mo = 0, argmax = 0;
    for (int b = 0; b < ctx->nblk; ++b) {
        si += hi[b];
        so += ho[b];
        if (hi[b] > mi) {
            mi = hi[b];
            argmax = b;
        }
        mo = std::max(mo, ho[b]);
    }
    fprintf(stderr, "[mdhip] tile halos: outer mean %.0f max %d; inner mean %.0f max %d (tile %d of %d); cap %d; rc %.3f skin %.3f inner skin %.3f\n",
            (double)so / ctx->nblk, mo, (double)si / ctx->nblk, mi, argmax, ctx->nblk, ctx->hcap_in, ctx->rc, ctx->skin,
            ctx->inner_skin);
}

// The fused form of md_dom_run_window (md_domain.hpp, "Fused slab step"): records in, nsteps x (k_step_tile, k_dom_post,
// all-reduce, record exchange, k_dom_adopt), records out.  The state is canonical (pos / v / f arrays) before and
// after the call, so list builds, downloads and the caller's planner see what they always saw; after a violation at
// step m the state returned is that of the last complete step, m - 1, and the caller resumes AT step m (info[6] = 1).
static bool dom_fused_available(md_ctx *c)
{
    return c->dom.on && c->dom.comm && c->allow_fused && c->use_tiles && c->virtual_ghosts && c->pot_kind != POT_CUSTOM &&
           c->skin > 0.0;
}

static void dom_exchange_records(md_ctx *ctx, double **sb, double **rb)
{
    auto &d = ctx->dom;
    hipStream_t st = ctx->stream;
    const int left = (d.rank + d.nranks - 1) % d.nranks, right = (d.rank + 1) % d.nranks;
    // (order: see md_dom_run_window -- with one or two ranks both neighbours are the same peer)
    g_rccl.check(g_rccl.GroupStart(), "ncclGroupStart");
    if (d.nsend_halo[0] > 0) g_rccl.check(g_rccl.Send(sb[0], 6 * d.nsend_halo[0], ncclFloat64, left, d.comm, st), "ncclSend");
    if (d.nsend_halo[1] > 0) g_rccl.check(g_rccl.Send(sb[1], 6 * d.nsend_halo[1], ncclFloat64, right, d.comm, st), "ncclSend");
    if (d.nrecv_halo[1] > 0) g_rccl.check(g_rccl.Recv(rb[1], 6 * d.nrecv_halo[1], ncclFloat64, right, d.comm, st), "ncclRecv");
    if (d.nrecv_halo[0] > 0) g_rccl.check(g_rccl.Recv(rb[0], 6 * d.nrecv_halo[0], ncclFloat64, left, d.comm, st), "ncclRecv");
    g_rccl.check(g_rccl.GroupEnd(), "ncclGroupEnd");
}

static int dom_run_window_fused(md_ctx *ctx, int64_t nsteps, double dt, int ensemble, double tau, double nf,
                                const double *ktemp, const double *r1, const double *r2, int report_last,
                                int apply_pending_scale, int64_t prune_interval, int32_t *first_viol, double *uwk,
                                double *info)
{
    auto &d = ctx->dom;
    int rc = md_dom_async_begin(ctx, nsteps, dt, ensemble, tau, nf, ktemp, r1, r2, prune_interval, d.own_flag.p,
                                d.own_kuw.p);
    if (rc != 0) return rc;
    hipStream_t st = ctx->stream;
    const bool nvt = d.a_nvt;
    const int n0s = (int)d.nsend_halo[0], n1s = (int)d.nsend_halo[1];
    const int n0r = (int)d.nrecv_halo[0], n1r = (int)d.nrecv_halo[1];
    const double shift_l = (d.rank == 0) ? ctx->L[0] : 0.0;
    const double shift_r = (d.rank == d.nranks - 1) ? -ctx->L[0] : 0.0;
    double *sb[2], *rb[2];
    for (int sd = 0; sd < 2; ++sd) {
        sb[sd] = (d.ext_cap >= 6 * d.nsend_halo[sd]) ? d.ext_send[sd] : d.sbuf[sd].p;
        rb[sd] = (d.ext_cap >= 6 * d.nrecv_halo[sd]) ? d.ext_recv[sd] : d.rbuf[sd].p;
    }
    const int planes = fused_uniform(ctx) ? 3 : 4;
    const size_t rs = rec_stride(ctx);
    const int post_grid = 1 + nblocks(std::max(n0s + n1s, 1));
    const int adopt_grid = nblocks(std::max(n0r + n1r, 1));
    // direct peer exchange (agreed for this window by md_dom_run_window): the post stores into the peers' mailboxes, the
    // adopt waits on this rank's own -- no collective in between
    const bool p2p = d.p2p.on && d.p2p.window;
    auto post = [&](int t, int want, const double2 *rec, int what, bool new_exchange = true) {
        P2pPut pa{};
        double *o0 = sb[0], *o1 = sb[1];
        if (p2p) {
            // (one exchange = its posts -- records and sums may go out in two launches -- and one adopt, all under one number)
            if (new_exchange) d.p2p.seq += 1;
            pa = dom_p2p_put_args(ctx, d.p2p.seq);
            o0 = dom_p2p_send_plane(ctx, 0, d.p2p.seq);
            o1 = dom_p2p_send_plane(ctx, 1, d.p2p.seq);
        }
        k_dom_post<<<(what & 2) ? post_grid : 1, MD_BLOCK, 0, st>>>(ctx->n > 0 ? ctx->nblk : 0, ctx->partials.p, want, d.kuw_dev,
                                                                    ctx->scal.p, t, n0s, n1s, d.send_slot[0].p, d.send_slot[1].p,
                                                                    rec, rs, shift_l, shift_r, o0, o1, what, pa);
    };
    // ... and both halves in one launch when the whole grid is resident at once (md_domain.hpp k_dom_exchange)
    const int xchg_grid = std::max(post_grid, adopt_grid);
    const bool merged = p2p && xchg_grid <= 1024 && !getenv("MDHIP_DOM_P2P_SPLIT");
    auto exchange = [&](int t, int want, double2 *rec, int finalize) {
        d.p2p.seq += 1;
        DomPostArgs pa{};
        pa.nblk = ctx->n > 0 ? ctx->nblk : 0;
        pa.partials = ctx->partials.p;
        pa.kuw4 = d.kuw_dev;
        pa.n0 = n0s;
        pa.n1 = n1s;
        pa.slot0 = d.send_slot[0].p;
        pa.slot1 = d.send_slot[1].p;
        pa.shift0 = shift_l;
        pa.shift1 = shift_r;
        pa.out0 = dom_p2p_send_plane(ctx, 0, d.p2p.seq);
        pa.out1 = dom_p2p_send_plane(ctx, 1, d.p2p.seq);
        pa.post_blocks = post_grid;
        DomAdoptArgs aa{};
        aa.n0 = n0r;
        aa.n1 = n1r;
        aa.xh_slot = d.xh_slot.p;
        aa.in0 = dom_p2p_recv_plane(ctx, 0, d.p2p.seq);
        aa.in1 = dom_p2p_recv_plane(ctx, 1, d.p2p.seq);
        aa.planes = planes;
        aa.pos = ctx->sb[ctx->cur].pos.p;
        aa.nvt = nvt ? 1 : 0;
        aa.nf = d.a_nf;
        aa.term1 = d.a_term1;
        aa.kt = ctx->d_kt.p;
        aa.r1 = ctx->d_r1.p;
        aa.r2 = ctx->d_r2.p;
        aa.adopt_blocks = adopt_grid;
        k_dom_exchange<<<xchg_grid, MD_BLOCK, 0, st>>>(pa, aa, rec, rec, rs, want, ctx->scal.p, t, finalize,
                                                       dom_p2p_put_args(ctx, d.p2p.seq), dom_p2p_get_args(ctx, d.p2p.seq, d.p2p.timeout));
    };
    auto collectives = [&](bool sums) {
        if (p2p) return;
        if (sums)
            g_rccl.check(g_rccl.AllReduce(d.kuw_dev, d.kuw_dev, 4, ncclFloat64, ncclSum, d.comm, st), "ncclAllReduce(K,U,W,viol)");
        dom_exchange_records(ctx, sb, rb);
    };
    // MDHIP_DOM_OVERLAP=1: the record exchange overlaps the interior tiles.  Off by default: with ONE rank (the only
    // configuration this code has been timed in) the exchange is a local copy and the two extra stream hand-overs per step
    // cost more than it hides -- 0.231 against 0.199 ms/step, profiles/r02_slab_overlap_world1.txt; DESIGN.md section 6.
    const char *ov = getenv("MDHIP_DOM_OVERLAP");
    const bool overlap = ov && ov[0] == '1' && d.n_tiles_i > 0 && d.n_tiles_b + d.n_tiles_i == ctx->nblk;
    if (overlap && !d.stream_i) {
        // (a priority of its own: the runtime then gives it a hardware queue of its own, so that the interior tiles
        // really run beside the boundary stream's kernels)
        int plo = 0, phi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&plo, &phi));
        HIPCHK(hipStreamCreateWithPriority(&d.stream_i, hipStreamNonBlocking, plo));
        HIPCHK(hipEventCreateWithFlags(&d.ev_go, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&d.ev_int, hipEventDisableTiming));
    }
    auto adopt = [&](int t, int want, double2 *rec, int finalize) {
        P2pGet ga{};
        const double *i0 = rb[0], *i1 = rb[1];
        if (p2p) {
            ga = dom_p2p_get_args(ctx, d.p2p.seq, d.p2p.timeout);
            i0 = dom_p2p_recv_plane(ctx, 0, d.p2p.seq);
            i1 = dom_p2p_recv_plane(ctx, 1, d.p2p.seq);
        }
        k_dom_adopt<<<adopt_grid, MD_BLOCK, 0, st>>>(n0r, n1r, d.xh_slot.p, i0, i1, rec, rs, planes,
                                                     ctx->sb[ctx->cur].pos.p, d.kuw_dev, want, nvt ? 1 : 0, d.a_nf, d.a_term1,
                                                     ctx->d_kt.p, ctx->d_r1.p, ctx->d_r2.p, ctx->scal.p, t, finalize, ga);
    };
    ctx->part = md_ctx::StepPart{}; // (a window that failed half-way may have left a part selected)
    // records of the state the window starts from: own particles from the arrays, the x-halo particles' from their owners
    FusedScope fscope{ctx};
    fused_enter(ctx, dt);
    if (merged) {
        exchange(-1, 0, ctx->rec[0].p, 0);
    } else {
        post(-1, 0, ctx->rec[0].p, 3); // (step -1 < every first_viol: packs; its sums are not used)
        collectives(false);
        adopt(-1, 0, ctx->rec[0].p, 0);
    }
    // MDHIP_DEBUG_DOM=1: wait after every stage and say so (finds the stage a rank is stuck in)
    const bool trace = getenv("MDHIP_DEBUG_DOM") != nullptr;
    int64_t t_now = 0;
    auto stage = [&](const char *what) {
        if (!trace) return;
        HIPCHK(hipStreamSynchronize(st));
        fprintf(stderr, "[mdhip] rank %d window step %lld: %s done\n", d.rank, (long long)t_now, what);
    };
    // MDHIP_DOM_FAIL="rank:step": this rank fails inside the window at that step (tests: its peers must error out through
    // the aborted communicator, not wait for a collective that never comes)
    // "rank:step:seconds": that rank stalls for so long instead (host sleep with the device idle): its peers' bounded
    // waits must end with the time-limit error (MDHIP_P2P_TIMEOUT_S), and the late rank must find the poison they left
    int fail_rank = -1, fail_step = -1;
    double fail_sleep = 0.0;
    if (const char *e = getenv("MDHIP_DOM_FAIL")) (void)sscanf(e, "%d:%d:%lf", &fail_rank, &fail_step, &fail_sleep);
    if (nsteps > 0) d.xhalo_pos_stale = true;
    for (int64_t t = 0; t < nsteps; ++t) {
        t_now = t;
        if (d.rank == fail_rank && t == fail_step) {
            if (!(fail_sleep > 0.0)) throw HipError("md_dom_run_window: injected failure (MDHIP_DOM_FAIL)");
            HIPCHK(hipStreamSynchronize(st));
            fprintf(stderr, "[mdhip] rank %d: injected stall of %.1f s (MDHIP_DOM_FAIL)\n", d.rank, fail_sleep);
            usleep((useconds_t)(fail_sleep * 1e6));
            fail_rank = -1; // (once)
        }
        const int want = (report_last && t == nsteps - 1) ? 1 : 0;
        // inner rows: the schedule (identical on every rank) is the caller's prune interval
        if (ctx->prune_on && ctx->inner_valid && d.w_prune_interval > 0 && ctx->steps_since_prune >= d.w_prune_interval)
            ctx->inner_valid = false;
        if (ctx->prune_on && !ctx->inner_valid) d.w_prune_steps.push_back((int)t);
        if (ctx->n > 0 && overlap) {
            // boundary tiles first, on the main stream; the interior tiles on their own stream while the boundary
            // particles' records are packed and travel; the sums (and so the all-reduce) wait for both
            const bool prune_step = ctx->prune_on && !ctx->inner_valid;
            if (prune_step) k_reset_d1<<<1, 1, 0, st>>>(ctx->scal.p, (int)t - 1);
            HIPCHK(hipEventRecord(d.ev_go, st));
            HIPCHK(hipStreamWaitEvent(d.stream_i, d.ev_go, 0));
            prof_begin(ctx, prune_step ? 3 : 0);
            ctx->part.list = d.tiles_b.p;
            ctx->part.count = d.n_tiles_b;
            ctx->part.stream = st;
            ctx->part.last = false;
            launch_step(ctx, want != 0, dt, (int)t);
            ctx->part.list = d.tiles_i.p;
            ctx->part.count = d.n_tiles_i;
            ctx->part.stream = d.stream_i;
            ctx->part.last = true;
            launch_step(ctx, want != 0, dt, (int)t);
            ctx->part = md_ctx::StepPart{};
            HIPCHK(hipEventRecord(d.ev_int, d.stream_i));
            double2 *recB = ctx->rec[ctx->fz_a].p; // the set this step wrote
            post((int)t, want, recB, 2);
            if (!p2p) dom_exchange_records(ctx, sb, rb);
            HIPCHK(hipStreamWaitEvent(st, d.ev_int, 0));
            prof_end(ctx); // (boundary tiles + pack + exchange, or the interior tiles: whichever took longer)
            stage("step + exchange");
            post((int)t, want, recB, 1, false);
            if (!p2p)
                g_rccl.check(g_rccl.AllReduce(d.kuw_dev, d.kuw_dev, 4, ncclFloat64, ncclSum, d.comm, st), "ncclAllReduce(K,U,W,viol)");
            adopt((int)t, want, recB, 1);
            stage("sums + all-reduce + adopt");
        } else {
            if (ctx->n > 0) {
                launch_step(ctx, want != 0, dt, (int)t);
            } else {
                ctx->fz_a ^= 1;
                if (ctx->prune_on && !ctx->inner_valid) {
                    ctx->inner_valid = true;
                    ctx->steps_since_prune = 0;
                }
            }
            double2 *recB = ctx->rec[ctx->fz_a].p; // the set this step wrote
            stage("step");
            if (merged) {
                exchange((int)t, want, recB, 1);
            } else {
                post((int)t, want, recB, 3);
                stage("post");
                collectives(true);
                adopt((int)t, want, recB, 1);
            }
            stage("exchange + adopt");
        }
        ctx->st_steps += 1;
        ctx->steps_since_prune += 1;
    }
    HIPCHK(hipGetLastError());
    Scalars h = read_scalars(ctx);
    if (h.comm_error != 0)
        throw HipError(h.comm_error == 2 ? "md_dom_run_window: a peer rank failed inside the window (direct peer exchange)"
                                         : "md_dom_run_window: a peer rank did not deliver within the time limit (direct peer "
                                           "exchange; MDHIP_P2P_TIMEOUT_S)");
    const int64_t fv = h.first_viol;
    const bool violated = fv < nsteps;
    if (violated) {
        // steps [0, fv) are complete; step fv read the buffer set that holds the state of step fv - 1: fall back to it
        const int a_start = (int)((ctx->fz_a ^ (int)(nsteps & 1)) & 1);
        ctx->fz_a = a_start ^ (int)(fv & 1);
        ctx->st_steps -= (nsteps - fv);
    }
    const bool swapped = ctx->fz_a != 0;
    fused_leave(ctx, nvt && apply_pending_scale && !violated);
    fscope.done = true;
    if (swapped && n0r + n1r > 0)
        k_dom_copy_xhalo<<<nblocks(n0r + n1r), MD_BLOCK, 0, st>>>(n0r + n1r, d.xh_slot.p, ctx->sb[ctx->cur ^ 1].pos.p,
                                                                 ctx->sb[ctx->cur].pos.p);
    if (nvt && apply_pending_scale && !violated) k_set_scale<<<1, 1, 0, st>>>(ctx->scal.p, 1.0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (first_viol) *first_viol = h.first_viol;
    if (uwk) {
        uwk[0] = h.U;
        uwk[1] = h.W;
        uwk[2] = h.K;
    }
    const int64_t done = violated ? fv : nsteps;
    debug_tile_halos(ctx);
    if (getenv("MDHIP_DEBUG"))
        fprintf(stderr, "[mdhip] rank %d fused window: %lld steps, first_viol=%lld, since build %lld, prunes in window %zu\n", d.rank,
                (long long)nsteps, (long long)fv, (long long)d.w_b0, d.w_prune_steps.size());
    ctx->steps_since_build = d.w_b0 + done;
    bool was_prune = false;
    int last_prune = -1;
    for (int p : d.w_prune_steps) {
        if (p == fv) was_prune = true;
        if (p < fv && p < nsteps) last_prune = p;
    }
    if (info) {
        double d12;
        unsigned long long bits = h.d1max2_bits;
        memcpy(&d12, &bits, sizeof d12);
        info[0] = was_prune ? 1.0 : 0.0;
        info[1] = std::sqrt(d12);
        info[2] = last_prune >= 0 ? (double)(d.w_b0 + last_prune + 1) : -1.0;
        info[3] = ctx->prune_on ? 1.0 : 0.0;
        info[4] = ctx->skin;
        info[5] = ctx->prune_on ? ctx->inner_skin : 0.0;
        info[6] = p2p ? 2.0 : 1.0; // fused window (2: over the direct peer exchange): after a violation nothing of step
                                   // first_viol is applied -- resume AT it
    }
    return 0;
}

int md_dom_run_window(md_ctx *ctx, int64_t nsteps, double dt, int ensemble, double tau, double nf, const double *ktemp,
                      const double *r1, const double *r2, int report_last, int apply_pending_scale,
                      int64_t prune_interval, int32_t *first_viol, double *uwk, double *info)
{
    API_BEGIN
    require_state(ctx, "md_dom_run_window");
    dom_require(ctx);
    auto &d = ctx->dom;
    if (!d.comm) throw HipError("md_dom_run_window: no communicator (md_dom_comm_init first)");
    DomAbortGuard guard{ctx};
    if (info) info[6] = 0.0;
    {
        // the fused and the classic window exchange different things: every rank takes the fused one or none does
        // (a rank whose tiles did not fit the LDS at the last list build walks the generic rows)
        int32_t hf = dom_fused_available(ctx) ? 1 : 0;
        if (hf && d.p2p.on) {
            // 2: the direct peer exchange can carry this window (the record planes hold what the last build counted)
            const int left = (d.rank + d.nranks - 1) % d.nranks, right = (d.rank + 1) % d.nranks;
            if (d.nsend_halo[0] <= d.p2p.peer_cap[left] && d.nsend_halo[1] <= d.p2p.peer_cap[right] &&
                d.nrecv_halo[0] <= d.p2p.cap && d.nrecv_halo[1] <= d.p2p.cap)
                hf = 2;
        }
        hipStream_t st = ctx->stream;
        HIPCHK(hipMemcpyAsync(d.own_flag.p, &hf, sizeof hf, hipMemcpyHostToDevice, st));
        g_rccl.check(g_rccl.AllReduce(d.own_flag.p, d.own_flag.p, 1, ncclInt32, ncclMin, d.comm, st), "ncclAllReduce(path)");
        HIPCHK(hipMemcpyAsync(&hf, d.own_flag.p, sizeof hf, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ctx->last_run_fused = hf >= 1;
        d.p2p.window = hf == 2;
    }
    if (getenv("MDHIP_DEBUG"))
        fprintf(stderr, "[mdhip] rank %d md_dom_run_window: %lld steps fused=%d (tiles=%d virtual_ghosts=%d allow=%d) since build %lld inner_valid=%d\n",
                d.rank, (long long)nsteps, (int)ctx->last_run_fused, (int)ctx->use_tiles, (int)ctx->virtual_ghosts, (int)ctx->allow_fused,
                (long long)ctx->steps_since_build, (int)ctx->inner_valid);
    if (ctx->last_run_fused) {
        if (d.own_kuw.n < 4) throw HipError("md_dom_run_window: internal: K/U/W buffer too small");
        int rcf = dom_run_window_fused(ctx, nsteps, dt, ensemble, tau, nf, ktemp, r1, r2, report_last, apply_pending_scale,
                                       prune_interval, first_viol, uwk, info);
        if (rcf == 0) guard.armed = false;
        return rcf;
    }
    int rc = md_dom_async_begin(ctx, nsteps, dt, ensemble, tau, nf, ktemp, r1, r2, prune_interval, d.own_flag.p,
                                d.own_kuw.p);
    if (rc != 0) return rc;
    hipStream_t st = ctx->stream;
    const int left = (d.rank + d.nranks - 1) % d.nranks, right = (d.rank + 1) % d.nranks;
    const bool nvt = d.a_nvt;
    for (int64_t t = 0; t < nsteps; ++t) {
        int want = (report_last && t == nsteps - 1) ? 1 : 0;
        rc = md_dom_step_a(ctx, dt, (int)t);
        if (rc != 0) return rc;
        // (the flag's all-reduce shares one group -- one launch -- with the halo exchange)
        const bool grouped = g_dom_group_flag;
        if (!grouped)
            g_rccl.check(g_rccl.AllReduce(d.flag_dev, d.flag_dev, 1, ncclInt32, ncclMin, d.comm, st), "ncclAllReduce(flag)");
        // halo coordinates to the two ring neighbours.  With one or two ranks both neighbours are the same
        // peer: messages between a pair match in issue order, and a rank's left-bound message is what its
        // peer receives "from the right" -- hence receive-from-right is posted first.
        double *sb[2], *rb[2];
        for (int sd = 0; sd < 2; ++sd) {
            sb[sd] = (d.ext_cap >= 3 * d.nsend_halo[sd]) ? d.ext_send[sd] : d.sbuf[sd].p;
            rb[sd] = (d.ext_cap >= 3 * d.nrecv_halo[sd]) ? d.ext_recv[sd] : d.rbuf[sd].p;
        }
        g_rccl.check(g_rccl.GroupStart(), "ncclGroupStart");
        if (grouped)
            g_rccl.check(g_rccl.AllReduce(d.flag_dev, d.flag_dev, 1, ncclInt32, ncclMin, d.comm, st), "ncclAllReduce(flag)");
        if (d.nsend_halo[0] > 0) g_rccl.check(g_rccl.Send(sb[0], 3 * d.nsend_halo[0], ncclFloat64, left, d.comm, st), "ncclSend");
        if (d.nsend_halo[1] > 0) g_rccl.check(g_rccl.Send(sb[1], 3 * d.nsend_halo[1], ncclFloat64, right, d.comm, st), "ncclSend");
        if (d.nrecv_halo[1] > 0) g_rccl.check(g_rccl.Recv(rb[1], 3 * d.nrecv_halo[1], ncclFloat64, right, d.comm, st), "ncclRecv");
        if (d.nrecv_halo[0] > 0) g_rccl.check(g_rccl.Recv(rb[0], 3 * d.nrecv_halo[0], ncclFloat64, left, d.comm, st), "ncclRecv");
        g_rccl.check(g_rccl.GroupEnd(), "ncclGroupEnd");
        rc = md_dom_step_b(ctx, dt, (int)t, want);
        if (rc != 0) return rc;
        if (nvt || want) {
            g_rccl.check(g_rccl.AllReduce(d.kuw_dev, d.kuw_dev, 3, ncclFloat64, ncclSum, d.comm, st), "ncclAllReduce(K,U,W)");
            // the scalar kernel only where its results are read by the host or by the next window; in between the
            // next kick-drift forms the Bussi scale from the reduced sums itself
            if (want || t == nsteps - 1) {
                rc = md_dom_step_c(ctx, (int)t, want);
                if (rc != 0) return rc;
            }
        }
    }
    guard.armed = false;
    return md_dom_async_end(ctx, apply_pending_scale, first_viol, uwk, info);
    API_END
}

// the Bussi scale computed by the caller from the all-reduced kinetic energy; applied in front of
// the next half-kick (src/thermostat.jl:43-45)
int md_dom_set_scale(md_ctx *ctx, double scale)
{
    API_BEGIN
    dom_require(ctx);
    k_set_scale<<<1, 1, 0, ctx->stream>>>(ctx->scal.p, scale);
    HIPCHK(hipGetLastError());
    API_END
}

// The whole list build of a slab handle in one call, the neighbour exchanges on the handle's own communicator:
// md_dom_migrate_pack -> counts + migrants -> md_dom_migrate_unpack -> md_dom_halo_pack -> counts + halo records ->
// md_dom_halo_unpack -> md_dom_build.  Collective.  Inner rows need the tiled kernel on every rank (the prune steps are
// scheduled once for all ranks): if some rank's build fell back, pruning is switched off everywhere and the build repeated.
int md_dom_rebuild(md_ctx *ctx)
{
    API_BEGIN
    require_state(ctx, "md_dom_rebuild");
    dom_require(ctx);
    auto &d = ctx->dom;
    if (!d.comm) throw HipError("md_dom_rebuild: no communicator (md_dom_comm_init first)");
    DomAbortGuard guard{ctx};
    auto sub = [&](int rc) {
        if (rc != 0) throw HipError(ctx->err);
    };
    for (int attempt = 0;; ++attempt) {
        int64_t ns[2] = {0, 0}, nr[2] = {0, 0};
        sub(md_dom_migrate_pack(ctx, ns));
        dom_exchange_var(ctx, ns, MD_MIG_REC, nr);
        sub(md_dom_migrate_unpack(ctx, nr));
        sub(md_dom_halo_pack(ctx, ns));
        dom_exchange_var(ctx, ns, MD_HALO_REC, nr);
        sub(md_dom_halo_unpack(ctx, nr));
        sub(md_dom_build(ctx));
        // (every rank asked for inner rows or none did: prune_enabled is set by the same caller code on all of them)
        if (!d.prune_enabled || attempt > 0) break;
        hipStream_t st = ctx->stream;
        int32_t hf = ctx->prune_on ? 1 : 0;
        HIPCHK(hipMemcpyAsync(d.own_flag.p, &hf, sizeof hf, hipMemcpyHostToDevice, st));
        g_rccl.check(g_rccl.AllReduce(d.own_flag.p, d.own_flag.p, 1, ncclInt32, ncclMin, d.comm, st), "ncclAllReduce(inner rows)");
        HIPCHK(hipMemcpyAsync(&hf, d.own_flag.p, sizeof hf, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (hf == 1) break;
        d.prune_enabled = false;
        ctx->list_valid = false;
    }
    guard.armed = false;
    API_END
}

int md_dom_counts(md_ctx *ctx, int64_t *out /* [8]: n_own, nsend_halo L/R, nrecv_halo L/R, n_ghost, tiled, pruning */)
{
    API_BEGIN
    dom_require(ctx);
    out[0] = ctx->n;
    out[1] = ctx->dom.nsend_halo[0];
    out[2] = ctx->dom.nsend_halo[1];
    out[3] = ctx->dom.nrecv_halo[0];
    out[4] = ctx->dom.nrecv_halo[1];
    out[5] = ctx->nghost;
    out[6] = ctx->use_tiles ? 1 : 0;
    out[7] = ctx->prune_on ? 1 : 0;
    API_END
}

} // extern "C"
