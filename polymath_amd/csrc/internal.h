// Internal declarations shared by the translation units of libpolymath_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/polymath_hip.h"
#include "../host/key_plan.hpp"
#include "../host/solve_plan.hpp"
#include "ec.cuh"

namespace pm {

// ---- error plumbing: every HIP failure becomes PM_ERR_HIP with a message, never an abort ----
struct pm_error_sink {
    std::string msg;
};

#define PM_HIP(ctx, expr)                                                                        \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e) + " @" + __FILE__ + ":" + \
                         std::to_string(__LINE__);                                               \
            return PM_ERR_HIP;                                                                   \
        }                                                                                        \
    } while (0)

#define PM_TRY(expr)                  \
    do {                              \
        int _s = (expr);              \
        if (_s != PM_OK) return _s;   \
    } while (0)

// a kernel launch and its launch-error check
#define PM_LAUNCH(ctx, kernel, grid, block, lds, stream, ...)                  \
    do {                                                                       \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);     \
        PM_HIP(ctx, hipGetLastError());                                        \
    } while (0)

// A runtime pm_curve id as a type: with_curve(curve, [&](auto cv) { return f<type_of<decltype(cv)>>(...); }) calls the lambda with a tag
// whose ::type is BlsCurve or BnCurve; any other id is PM_ERR_INVALID_ARG.  (host/polymath.hpp: with_transcript does the same for the
// three host transcripts.)
template <class C>
struct CurveTag { typedef C type; };
template <class Tag>
using type_of = typename Tag::type;
template <class F>
inline int with_curve(int curve, F f) {
    if (curve == PM_BLS12_381) return f(CurveTag<BlsCurve>{});
    if (curve == PM_BN254) return f(CurveTag<BnCurve>{});
    return PM_ERR_INVALID_ARG;
}

// Growable device buffer owned by a context (never shrinks: the prover reuses its workspaces).
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            if (e != hipSuccess) return e;
            p = nullptr;
            bytes = 0;
        }
        size_t want = need + need / 8;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, need);
            want = need;
        }
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T *as() const { return (T *)p; }
    // v to the buffer's start, grown to hold it, by an asynchronous copy on `stream` (v must live until it has run); an empty v
    // touches nothing
    template <class T>
    hipError_t upload(const std::vector<T> &v, hipStream_t stream) {
        if (v.empty()) return hipSuccess;
        const hipError_t e = reserve(v.size() * sizeof(T));
        return e != hipSuccess ? e : hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream);
    }
};

// A DevBuf that lives for one call: released on every way out of its scope.  DevBuf itself has no destructor because the context's
// workspaces (pm_ctx, pm_bases) release explicitly; every call-scoped buffer is one of these.
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    void operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { release(); }
};

enum TimingSlot {
    T_WITNESS_MAP = 0,
    T_NTT = 1,
    T_POLY = 2,
    T_MSM_SORT = 3,
    T_MSM_ACCUMULATE = 4,
    T_MSM_REDUCE = 5,
    T_MSM_TOTAL = 6,
    T_PHASE = 7,
    T_NUM_SLOTS = 8,
    // the batch verifier's names for the same slots (api.py: VERIFY_TIMING_SLOTS)
    TV_DECODE = T_WITNESS_MAP,
    TV_TERMS = T_NTT,
    TV_TREE = T_POLY,
    TV_HOST_GLUE = T_MSM_SORT,             // wall ms of the host's part of the challenges stage
    TV_PAIRING_HOST = T_MSM_ACCUMULATE,    // wall ms of the pairing stage
    TV_PAIRING_KERNELS = T_MSM_REDUCE,
    TV_CHALLENGE_KERNEL = T_MSM_TOTAL,
    TV_DEVICE_TOTAL = T_PHASE
};

// What one bucket pipeline hands from its sort to its accumulation and from there to the reduction.
struct MsmSet {
    DevBuf sorted, counts, bucket_off, task_off, tasks, partials, task_cnt;   // tasks: uint4 descriptors in accumulate order (msm.hip: k_task_bins)
};
struct MsmWorkspace {
    MsmSet set;
    DevBuf digits, cursor, wsum, region, sub, digits2, len_bins, block_cnt, hot;
    DevBuf batch;   // msm_run_batch: the base range's infinity flags, then (host form) one (point, flag) record per row of the batch
};
inline size_t batch_flag_bytes(size_t len) { return (len + 15) & ~(size_t)15; }

// Window tables of a resident base vector (setup.hip: tables_build) or, with wide, the plan of an MSM that runs without tables: the
// layout (msm_plan.h: WindowLayout -- planned(), widest(), the bucket sets) plus where the points are.  Point (w, i) lives at index
// w * stride + i of the table array.  Not planned: no tables (per-window Pippenger).
struct MsmTables : WindowLayout {
    size_t stride = 0;               // points per window (0 in wide mode)
    size_t base_index = 0;           // first point of this MSM inside window 0
    const unsigned char *inf = nullptr;   // device: one flag byte per point of window 0 (1 = point at infinity)
    const void *table = nullptr;          // device: TablePoint<C>[nwin][stride]; nullptr in wide mode
    MsmTables() = default;
    MsmTables(const WindowLayout &layout, size_t points_per_window) : WindowLayout(layout), stride(points_per_window) {}
};

// The vectors of `rows` proofs against one unsharded key as [rows][len] arrays (prove.hip / prove_batch.hip), reserved for the largest
// shape seen and reused.  A context holds two: pm_ctx::pw, the proof in flight of the three-phase API (rows = 1; the sharded prover keeps
// its local vectors there too), and pm_ctx::pb, the groups of pm_host_prove_batch -- a batch call leaves the proof in flight alone.
struct ProveWs {
    // tmp: the transforms' out-of-place temporary; part: phase 2's partial sums; rows: the per-proof values of the phase being run
    // (phase 1: r_a as [rows][2], phases 2 and 3 of a group: one BatchRow record per proof); flags: one status word per proof
    DevBuf xw, ue, we, u, w, wit_u, u2, tmp, sc_a, sc_c, quotient, lvl[6], part, rows, flags;
    template <class F>
    void for_each(F f) {
        for (DevBuf *b : {&xw, &ue, &we, &u, &w, &wit_u, &u2, &tmp, &sc_a, &sc_c, &quotient, &part, &rows, &flags}) f(*b);
        for (DevBuf &b : lvl) f(b);
    }
    void release() { for_each([](DevBuf &b) { b.release(); }); }
    size_t bytes_held() {
        size_t held = 0;
        for_each([&](DevBuf &b) { held += b.bytes; });
        return held;
    }
};

// pm_host_prove_batch with PM_PROVE_GLUE_DEVICE (prove_glue.hip): what the glue kernels read and write for one group of proofs, and
// tap 11 for the whole call.  pts: the (point, flag) records of [a]_1, [c]_1, [d]_1 as three arrays of `cap` rows (the host-glue
// prover's phases leave theirs there too); inst: the hashed public inputs, [rows][m0]; ra: r_a as [rows][2]; keep: one record per
// proof from k_glue_x1 to the later kernels (the transcript's sponge among it); out: the group's proof bytes, then one status word
// per proof -- what the group's one copy brings down into `host`; tap: x1, x2, a(x1), c(x1) of all proofs of the last call.
struct GlueWs {
    DevBuf pts, inst, ra, keep, out, tap;
    size_t cap = 0;            // rows per array of pts
    size_t tap_rows = 0;       // pm_prove_tap(11): proofs of the last device-glue call; 0 = none
    std::vector<uint8_t> host, rows_host;   // rows_host: the host-glue prover's BatchRow records on their way up
    void release() {
        for (DevBuf *b : {&pts, &inst, &ra, &keep, &out, &tap}) b->release();
        cap = tap_rows = 0;
    }
};

// Witness solving (solve.hip): the context's plan cache -- one plan, keyed by (key, the key's hint generation, unknown pattern) -- and the buffers of the last
// call with PM_ASSIGNMENT_SOLVE.  xw: the completed x || w rows of a check call (pm_prove_tap(10)); the prover completes its groups in
// its own workspace (ProveWs::xw) and keeps only tap9.
struct SolveWs {
    DevBuf xw, pattern, mismatch, stuck, steps, bit_cols, pairs, divs, blocks, block_idx, block_inv, hints, hint_idx, mods, muls;
    pmsolve::Plan plan;
    // per plan.pairs / plan.divs / plan.blocks one record in `pairs` / `divs` / `blocks` (the blocks' rows and columns in `block_idx`,
    // their inverses in `block_inv`); plan.hints divides into the two record arrays that solve_plan counts:
    size_t n_hints = 0;                  // long divisions of the plan, wide ones included: records in `hints`, columns and literal divisors in `hint_idx`
    size_t n_mods = 0;                   // modular divisions of the plan: records in `mods`, columns and literal moduli in `hint_idx` as well
    size_t n_muls = 0;                   // modular multiply-divides of the plan: records in `muls`, columns and literal moduli in `hint_idx` as well
    uint64_t plan_key = 0;               // pm_pk::serial of the plan's key; 0 = no plan
    uint64_t plan_hint_gen = 0;          // pm_pk::hint_gen of the plan's key when the plan was made
    std::vector<uint8_t> plan_pattern;   // one byte per column
    std::vector<uint64_t> tap9;          // pm_prove_tap(9): per assignment 4 * (1 + m0) words; empty = no call with the flag yet
    size_t tap10_rows = 0;               // pm_prove_tap(10): rows of xw that hold a check call's completed assignments; 0 = none
    size_t tap10_cols = 0;
    void release() {
        for (DevBuf *b : {&xw, &pattern, &mismatch, &stuck, &steps, &bit_cols, &pairs, &divs, &blocks, &block_idx, &block_inv, &hints, &hint_idx, &mods, &muls}) b->release();
    }
};

struct TwiddleCache {
    int curve = -1;
    unsigned log_n = 0;
    unsigned long long stamp = 0;   // last use (LRU eviction)
    DevBuf fwd, inv;          // n/2 twiddles each, standard Montgomery form
    DevBuf fwd_int, inv_int;  // the same powers in the reduced-radix internal form (ntt.hip butterflies): dense 8 x u32 for the
                              // 32-bit-limb tile kernels, 10 x u32 28-bit-limb records for the 28-bit ones (ntt_l28_domain)
};

}  // namespace pm

struct pm_bases {
    int curve;
    int device;
    size_t len;
    void *d_points;  // Affine<C>[len], internal Montgomery form
    void *d_inf;     // infinity flags of the table set (tables.inf)
    void *d_table;   // TablePoint<C>[nwin][len] after pm_bases_precompute (tables.table)
    pm::MsmTables tables;
};

namespace pm {
uint64_t pk_serial_next();   // api.hip: 1, 2, 3, ... -- a key's identity for caches that outlive it (an address can come back)
}

// A resident proving key: the plan of host/key_plan.hpp (shapes, the logical base concatenation, this rank's pieces and segments --
// the provers read its fields as the key's) and the device memory that holds what it describes.
struct pm_pk : pm::KeyPlan {
    uint64_t serial = pm::pk_serial_next();
    int curve = 0, device = 0;
    uint64_t omega[4] = {0, 0, 0, 0};
    // the declared hints of the witness solver (pm_pk_set_hints): part of the circuit, like the matrices.  hint_gen changes with
    // every declaration (0: none was ever made), so that a plan made under another declaration is not reused
    std::vector<pmsolve::Hint> hints;
    uint64_t hint_gen = 0;
    // Every device allocation of the key is made by alloc() and freed by the destructor; the typed pointers below are views of them.
    std::vector<void *> owned;
    template <class T>
    hipError_t alloc(T **p, size_t bytes) {
        owned.reserve(owned.size() + 1);
        const hipError_t e = hipMalloc((void **)p, bytes);
        if (e == hipSuccess) owned.push_back((void *)*p);
        return e;
    }
    pm_pk() = default;
    pm_pk(const pm_pk &) = delete;
    void operator=(const pm_pk &) = delete;
    ~pm_pk() {
        (void)hipSetDevice(device);
        for (void *p : owned) (void)hipFree(p);
    }
    // R1CS matrices on the device (CSR; duplicates of a column inside a row removed, see api)
    uint64_t *d_rowptr[3] = {nullptr, nullptr, nullptr};
    uint32_t *d_col[3] = {nullptr, nullptr, nullptr};
    uint64_t *d_val[3] = {nullptr, nullptr, nullptr};
    uint64_t nnz[3] = {0, 0, 0};
    // the resident points of all base vectors in one allocation: the pieces of merged MSM k back to back from element res_dev_off[k]
    // (the whole concatenation in its own order when whole_resident()), so that every merged MSM reads one contiguous range
    void *d_bases = nullptr;
    uint64_t max_piece = (uint64_t)1 << 27;   // msm_max_piece of the creating context (pm_pk_msm_plan reports plans without a context)
    void *d_segs = nullptr;                   // device copy of `segs`
    void *d_all_segs = nullptr;               // device copy of `all_segs`
    // Window tables, ONE SET PER MERGED MSM (its own window width: the optimum depends on the pair count):
    // d_tab[k] holds [nwin_k][res_cnt[k]] points, window 0 being a copy of the MSM's resident pairs.
    pm::MsmTables tables[3];
    void *d_tab[3] = {nullptr, nullptr, nullptr}, *d_tab_inf[3] = {nullptr, nullptr, nullptr};   // tables and their infinity flags (tables[k].inf)
};

// One persistent host thread per context that runs a helper job (the overlapped [a]_1 MSM of prove.hip): created on first
// use, parked on a condition variable between proofs -- a std::thread per proof costs 30-50 us, which matters once a
// proof's share of an 8-GPU job is ~15 ms.
struct pm_worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = true, stop = false;
    bool submit(std::function<void()> fn) {      // false: the thread could not be created (caller runs the job inline)
        std::unique_lock<std::mutex> lk(mu);
        if (!th.joinable()) {
            try {
                th = std::thread([this] {
                    std::unique_lock<std::mutex> l(mu);
                    for (;;) {
                        cv.wait(l, [this] { return has_job || stop; });
                        if (stop) return;
                        std::function<void()> f = std::move(job);
                        has_job = false;
                        l.unlock();
                        f();
                        l.lock();
                        done = true;
                        cv.notify_all();
                    }
                });
            } catch (const std::system_error &) {
                return false;
            }
        }
        job = std::move(fn);
        has_job = true;
        done = false;
        cv.notify_all();
        return true;
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return done; });
    }
    ~pm_worker() {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this] { return done; });
            stop = true;
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }
};

// pm_option values of a context (include/polymath_hip.h); defaults and their environment names in api.hip: options_defaults
struct pm_options {
    long long v[PM_NUM_OPTIONS];
};

struct PendingTimer {
    int slot;
    hipEvent_t a, b;
};

struct pm_ctx {
    int device;
    pm_options opt;           // pm_ctx_set_option; the helper context `aux` carries a copy
    std::vector<PendingTimer> pending_timers;
    std::vector<hipEvent_t> event_pool;   // recycled stage-timer events: ~50 create / destroy pairs per proof are 0.2 ms of host time
    hipStream_t stream;
    std::string err;
    double timing_ms[pm::T_NUM_SLOTS];
    hipEvent_t ev_sc_a;       // recorded when the [a]_1 scalars are ready (prove.hip: the helper stream waits on it)
    pm::MsmWorkspace msm;
    pm::TwiddleCache tw[8];   // the sharded prover works with log m, log n and log 2n tables of both directions
    unsigned long long tw_clock;
    pm::DevBuf scratch, ntt_tmp;   // ntt_tmp: the out-of-place first / last passes of ntt_run
    void *h_pinned;           // 4 KiB of pinned host memory: the asynchronous MSM's result slot (msm.hip: msm_begin / msm_end)
    int msm_async;            // 0 none pending, 1 enqueued (msm_end synchronises), 2 ran synchronously (result parked in the slot)
    bool ntt_lds_attr[2];     // ntt.hip: the tile kernels' dynamic-LDS limit has been raised on this context's device (per curve id)
    pm_comm *comm;            // this rank's communicator (pm_ctx_set_comm); null on single-GPU contexts
    pm_worker worker;         // runs the helper context's MSM concurrently with this context's own work
    pm_ctx *aux;              // helper context (own stream + MSM workspace) for the second of two concurrent MSMs
    pm::DevBuf fb_table[2];   // setup.hip: 8-bit-window multiples of the G1 generator, per curve id (built on first use)
    // proof in flight
    const pm_pk *pk;
    int phase;
    std::vector<uint8_t> seg_all;   // sharded prover: phase 2's exchanged records ([u(x1) partial | P_s | Q_s] per rank) for phase 3
    uint64_t x1_host[4];      // ... and the x1 they were taken at
    uint64_t ra_host[8];      // r_a of the proof in flight (phase 3's numerator constants need it on the host)
    bool keep_timings;   // pm_host_prove: the stage slots accumulate over the three phases of one proof
    bool lazy_timings;   // ... and are read by pm_last_timings instead of at the end of every phase (timing_flush)
    pm::ProveWs pw;      // its vectors (prove.hip; prove_sharded.hip: this rank's local ones)
    // PM_SHARD_VECTOR prover (prove_sharded.hip): transform temporaries, halo coefficients, roots of the cross-rank butterfly
    pm::DevBuf sh_a, sh_b, sh_c, halo, shard_roots;
    pm::ProveWs pb;      // pm_host_prove_batch: the vectors of a group of proofs
    pm::SolveWs sv;
    pm::GlueWs gw;
    std::vector<uint64_t> verify_tap;   // pm_prove_tap(8): x1, x2, c(x1), ok of the last batch verified with device challenges, 16 words a proof
    uint64_t shard_roots_n;
    uint32_t shard_roots_N;
    int shard_roots_curve;
};

namespace pm {

// Developer aid: PM_PROFILE_HOST=1 prints, at the end of every phase of the sharded prover, how the HOST thread's wall time of that
// phase splits over labelled sections (stderr; one line per phase and rank).  What a kernel trace cannot show: waits, collectives,
// host arithmetic.  Costs two clock reads per section when off.
struct HostProfile {
    bool on;
    const char *phase;
    int rank;
    std::chrono::steady_clock::time_point t0, last;
    std::vector<std::pair<const char *, double>> parts;
    HostProfile(const char *ph, int r) : phase(ph), rank(r) {
        static const bool enabled = [] { const char *e = getenv("PM_PROFILE_HOST"); return e && e[0] == '1'; }();
        on = enabled;
        if (on) t0 = last = std::chrono::steady_clock::now();
    }
    void mark(const char *label) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        parts.emplace_back(label, std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    }
    ~HostProfile() {
        if (!on) return;
        std::string line = std::string("[pm host rank ") + std::to_string(rank) + "] " + phase + ":";
        char buf[96];
        for (auto &p : parts) { snprintf(buf, sizeof buf, " %s=%.3f", p.first, p.second); line += buf; }
        snprintf(buf, sizeof buf, " | total=%.3f ms\n", std::chrono::duration<double, std::milli>(last - t0).count());
        line += buf;
        fputs(line.c_str(), stderr);
    }
};

// PM_HOST_THREADS of the environment (read once, api.hip): the host glue's thread count; 0 = not set, the caller chooses
int host_threads_env();

// ---- per-curve entry points implemented in the .hip translation units -----------------------
template <class C>
int ntt_run(pm_ctx *ctx, Fp<typename C::FrP> *d_data, unsigned log_n, bool inverse);
// `rows` transforms, row b at d_data + b * row_stride, the row as grid y of ntt_run's passes (rows == 1: exactly ntt_run)
template <class C>
int ntt_run_batch(pm_ctx *ctx, Fp<typename C::FrP> *d_data, unsigned log_n, bool inverse, size_t rows, size_t row_stride);
// device table of omega_{2^log_n}^j (or its inverse), j < 2^(log_n - 1); cached per context
template <class C>
int twiddles_get(pm_ctx *ctx, unsigned log_n, bool inv_dir, const Fp<typename C::FrP> **out);

// tables == nullptr (or not planned): d_bases points at the MSM's first base.  Otherwise d_bases is unused, the
// points come from tables->table and tables->base_index locates the MSM's first base inside window 0.
template <class C>
int msm_run(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len,
            Affine<C> *h_out, int *h_inf, const MsmTables *tables = nullptr);

// `batch` MSMs of `len` pairs against the same bases: row b = d_scalars[b * len ..), results in h_out[b], h_inf[b].  Per-window pipeline
// over the plain base array only (no tables, no wide plan); see msm.hip.
template <class C>
int msm_run_batch(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len, size_t batch,
                  Affine<C> *h_out, int *h_inf);

// the same with row b's record left in d_out[b] (device memory): enqueued on ctx->stream, no copy to the host, no synchronisation;
// len <= msm_max_piece(ctx)
template <class C>
struct BatchPoint {
    Affine<C> p;       // standard Montgomery; x = y = 0 for the identity
    uint32_t inf;
};
template <class C>
int msm_run_batch_device(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len, size_t batch, BatchPoint<C> *d_out);

// the same in two halves (msm.hip): enqueue on ctx->stream without waiting / wait and convert
template <class C>
int msm_begin(pm_ctx *ctx, const Affine<C> *d_bases, const Fp<typename C::FrP> *d_scalars, size_t len, const MsmTables *tables);
template <class C>
int msm_end(pm_ctx *ctx, Affine<C> *h_out, int *h_inf);
template <class C>
int msm_resident_begin(pm_ctx *ctx, const pm_pk *pk, int which, const Fp<typename C::FrP> *d_scalars, uint64_t lo = 0, uint64_t count = 0);
template <class C>
int msm_resident_end(pm_ctx *ctx, uint64_t *out_xy, int *out_inf);

// msm_reduce.hip: the bucket reduction of the table-mode MSM over the sets of one ReduceShape (msm_plan.h; bucket_plan made and checked
// it) whose task partials sit in ctx->msm, three launches on ctx->stream; *out = the sums sum_b (b + 1) B_b of the sets, internal
// form, inside the workspace.  bucket0: first bucket of the first set.
template <class C>
int reduce_two_level(pm_ctx *ctx, const ReduceShape &shape, XYZZ<C> **out, size_t bucket0 = 0);

// One bucket pipeline covers at most this many pairs (sorted-entry positions are u32: windows x pairs < 2^32); longer
// MSMs run in pieces summed on the host.  2^27 in production; PM_OPT_MSM_MAX_PIECE_LOG (developer / test knob) lowers it
// so that the piece-split path can be exercised at small sizes.
inline size_t msm_max_piece(const pm_ctx *ctx) {
    const long long lg = ctx->opt.v[PM_OPT_MSM_MAX_PIECE_LOG];
    return (size_t)1 << (lg < 4 ? 4 : lg > 27 ? 27 : lg);
}

// window 0 of d_table <- the `count` internal-form affine points at d_points; then windows 1..nwin-1
template <class C>
struct TablePoint;   // fq28.cuh: 128-byte, 28-bit-limb record
template <class C>
int tables_build(pm_ctx *ctx, const Affine<C> *d_points, TablePoint<C> *d_table, size_t count, const MsmTables &t);
// flags[i] = 1 iff points[i] is the point at infinity (all-zero x, y)
template <class C>
int infinity_flags(pm_ctx *ctx, const Affine<C> *d_points, size_t count, unsigned char *d_flags);

template <class C>
int bases_generate_multiples(pm_ctx *ctx, size_t len, Affine<C> *d_out);

template <class C>
int fixed_base_batch(pm_ctx *ctx, const Fp<typename C::FrP> *d_scalars, size_t len, Affine<C> *d_out);

// Device base vectors are kept in the INTERNAL Montgomery radix of the reduced-radix accumulate kernel
// (fq28.cuh); this converts a device array in place at the API boundary (upload / generate / export).
template <class C>
int bases_convert(pm_ctx *ctx, Affine<C> *d_points, size_t len, bool to_internal);

// g1_codec.hip: compressed G1 (include/polymath_hip.h, pm_g1_status).  Decode: `count` records of 4 fq words each at d_in (16-byte
// aligned) -> standard-Montgomery affine points (refused and infinity: x = y = 0); d_status (optional) one pm_g1_status per point;
// d_first_bad (optional) atomically lowered to ((base_index + i) << 8 | status) for every refused point i.  Encode: the inverse,
// standard-Montgomery points -> records (d_out 16-byte aligned).  form = PM_WIRE_UNCOMPRESSED: records of 8 fq words (x || y), the
// same outputs and verdicts.
template <class C>
int g1_decode_device(pm_ctx *ctx, const uint8_t *d_in, size_t count, bool validate, Affine<C> *d_out, uint8_t *d_status,
                     unsigned long long *d_first_bad, uint64_t base_index, int form = PM_WIRE_COMPRESSED);
template <class C>
int g1_encode_device(pm_ctx *ctx, const Affine<C> *d_pts, size_t count, uint8_t *d_out, int form = PM_WIRE_COMPRESSED);
const char *g1_status_text(int curve, int status, int form = PM_WIRE_COMPRESSED);
template <class C>
constexpr size_t g1_record_bytes(int form) { return (size_t)4 * C::FqP::N * (form == PM_WIRE_UNCOMPRESSED ? 2 : 1); }

// pairing_batch.hip: checks  prod_j e(P[i][j], Q_j) == 1  against k <= 4 fixed G2 points, one lane per check.  pairing_prepare walks the
// Miller loop of each Q_j on the host (g2: k x 4 Fq, x.c0 || x.c1 || y.c0 || y.c1; bit j of `pairs` clear: Q_j = O, the pair is left out
// and its words are not read; a point off the twist is PM_ERR_INVALID_ARG) and uploads the line tables, which live as long as `out`.
// pairing_check_launch enqueues ONE launch of `count` lanes on the context's stream: lane i takes its k points from d_pts[i k ..], or,
// with d_terms (k == 3), from node i of the batch verifier's sum tree as U_i + neg_g_i G, -V_i, W_i (d_neg_g: 8 canonical words a
// lane; d_live: optional, a zero byte leaves the lane out).  d_is_one: one byte 0 / 1 per lane.  GPU ms go to timing_slot.
struct PairingPrepared {
    ScopedDevBuf buf;
    size_t consts_offset = 0;
    int k = 0;
    unsigned pairs = 0;
};
template <class C>
struct VerifyTerm;
template <class C>
int pairing_prepare(pm_ctx *ctx, const uint32_t *g2, int k, unsigned pairs, PairingPrepared *out);
template <class C>
int pairing_check_launch(pm_ctx *ctx, const PairingPrepared &prep, const Affine<C> *d_pts, const VerifyTerm<C> *d_terms, const uint32_t *d_neg_g,
                         const uint8_t *d_live, const Affine<C> &G, size_t count, uint8_t *d_is_one, int timing_slot);
// pairing_wave.hip: the same checks, one per group of 36 lanes of a wave (pairing_wave.cuh), on the tables of pairing_prepare.  With
// d_terms the launch also needs fixed_base_prepare's table of this call's G (the points d 2^(4 t) G), from which the lanes sum neg_g_i G.
// PM_VERIFY_PAIRING_DEVICE_WAVE checks the root this way, and the live leaves after a failing root while there are at most
// VERIFY_WAVE_LEAF_MAX of them (a wave a leaf; above that, a lane a leaf: pairing_check_launch).  1024 is a STARTING value, not a
// tuned one: the measured crossover lies near 12 000 live leaves on both curves (profiles/verify_batch_wave_pairing.txt), so anything
// up to 8192 would still gain.  polymath_amd/api.py mirrors it.
constexpr size_t VERIFY_WAVE_LEAF_MAX = 1024;
template <class C>
int fixed_base_prepare(pm_ctx *ctx, const Affine<C> &G, ScopedDevBuf *out);
template <class C>
int pairing_check_wave_launch(pm_ctx *ctx, const PairingPrepared &prep, const ScopedDevBuf &fixed_base, const Affine<C> *d_pts, const VerifyTerm<C> *d_terms,
                              const uint32_t *d_neg_g, const uint8_t *d_live, size_t count, uint8_t *d_is_one, int timing_slot);
// challenges.hip: the verifier's Fiat-Shamir challenges (transcript.cuh: fs_verifier_challenges), one proof per lane, ONE launch on
// the context's stream.  Proof i reads its [a]_1 / [c]_1 records at d_a + i a_stride / d_c + i c_stride, the 32 bytes of a(x1) at
// d_a_at + i a_at_stride and n_inputs Montgomery public inputs at d_inputs + i n_inputs (all strides multiples of 8, the bases
// 8-byte aligned).  Outputs, each optional (null: not written): x1, x2, c(x1) (Montgomery); ok (0: a(x1) >= r, the row's outputs
// are zero); and, with d_scalars -- whose rho words the caller has filled -- the batch verifier's record (rho x2, rho x1 canonical)
// and d_g[i] = rho_i (a(x1) + x2 c(x1)) (Montgomery); a row that is not ok, or one of whose three points the decoder refused
// (d_point_status: optional, 3 bytes a row), gets an all-zero record and g = 0: no weight, it never enters a sum.
// GPU ms go to timing_slot.
struct VerifyScalars;
struct ChallengeRows {
    const uint8_t *d_a, *d_c, *d_a_at;
    size_t a_stride, c_stride, a_at_stride;
    const uint64_t *d_inputs;
    size_t n_inputs, count;
    const uint8_t *d_point_status;
};
template <class C>
int verifier_challenges_launch(pm_ctx *ctx, int transcript, uint64_t n, uint64_t sigma, const Fp<typename C::FrP> &omega, const ChallengeRows &rows,
                               Fp<typename C::FrP> *d_x1, Fp<typename C::FrP> *d_x2, Fp<typename C::FrP> *d_c_at_x1, uint8_t *d_ok,
                               VerifyScalars *d_scalars, Fp<typename C::FrP> *d_g, int timing_slot);
// ProvingKey::serialize_compressed / serialize_uncompressed (form: pm_wire_form) parsed on the host without touching its base points (pk_wire_parse)
struct WireLayout {
    size_t vk_len = 0;
    uint64_t n = 0, vk_m0 = 0, sigma = 0, omega[4] = {0, 0, 0, 0};   // the vk's header fields
    uint64_t m0 = 0, mw = 0, nr = 0;                                  // the SAP matrices' header
    std::vector<uint64_t> rowptr[3], val[3];                          // a, b, c as serialised (duplicates kept), val Montgomery
    std::vector<uint32_t> col[3];
    uint64_t vec_off[PM_NUM_BASE_VECS] = {0}, vec_len[PM_NUM_BASE_VECS] = {0};   // by pm_base_vec: byte offset of point 0, points
    // the vk's points for the relation check (key_check.hip): one_g1 as x || y (standard Montgomery; all zero = infinity) and
    // [1]_2, [x]_2, [z]_2 packed as pairing_prepare reads them (4 Fq a point: x.c0 || x.c1 || y.c0 || y.c1); g2_inf: one of the three is the point at infinity
    uint32_t vk_one_g1[2 * 12] = {0}, vk_g2[3 * 4 * 12] = {0};
    bool vk_g2_inf = false;
};
template <class C>
int pk_wire_parse(const uint8_t *data, size_t len, int form, WireLayout &out, std::string &err);

// key_check.hip: PM_KEY_CHECK_RELATIONS.  Is the whole-resident key `pk`, its points decoded and validated but its tables not yet built,
// what generate_proving_key would have produced for some (x, z) under the vk (one_g1; g2 = [1]_2, [x]_2, [z]_2 as pairing_prepare
// reads them)?  *failed = the first failing relation (host/key_check.hpp: KeyRelation, key_relation_text) or KEY_REL_NONE.  seed: the 32
// bytes the weights are expanded from.  Synchronises the stream; its device memory, the MSM workspace included, is returned.
template <class C>
int key_check_run(pm_ctx *ctx, const pm_pk *pk, const Affine<C> &one_g1, const uint32_t *g2, const uint8_t seed[32], int *failed);

// setup.hip: the uj_wj_lcs scalars of generator.rs:112-136 on the device (Lagrange coefficients at x + the sparse pass over the
// key's CSR matrices); `lagrange` and `work` are the caller's scratch
template <class C>
int lcs_scalars(pm_ctx *ctx, const pm_pk *pk, const Fp<typename C::FrP> &x, const Fp<typename C::FrP> &omega, const Fp<typename C::FrP> &kscale,
                const Fp<typename C::FrP> &y_gamma, const Fp<typename C::FrP> &y_to_minus_alpha, DevBuf &lagrange, DevBuf &work,
                Fp<typename C::FrP> *d_lcs);

template <class C>
int powers_fill(pm_ctx *ctx, Fp<typename C::FrP> *d_out, size_t count, const Fp<typename C::FrP> &scale,
                const Fp<typename C::FrP> &x);

// MSM `which` (0 = a, 1 = c, 2 = d) over this rank's resident pairs; d_scalars in the order of pk->pieces[which]
template <class C>
int msm_resident(pm_ctx *ctx, const pm_pk *pk, int which, const Fp<typename C::FrP> *d_scalars, uint64_t *out_xy, int *out_inf);

// prove.hip: phase 1's enqueue list between the uploads and the MSMs, for the `rows` proofs of a ProveWs (both provers run it)
struct ProofShape;
template <class C>
int phase1_enqueue_u(pm_ctx *ctx, const pm_pk *pk, const ProofShape &shape, ProveWs &ws, size_t rows, bool sc_a_now);
template <class C>
int phase1_enqueue_rest(pm_ctx *ctx, const pm_pk *pk, const ProofShape &shape, ProveWs &ws, size_t rows, Fp<typename C::FrP> *sc_a_or_null);

template <class C>
int prove_phase1_impl(pm_ctx *ctx, const pm_pk *pk, const uint64_t *x, const uint64_t *w, const uint64_t *r_a,
                      uint64_t *a_xy, int *a_inf, uint64_t *c_xy, int *c_inf, bool assignment_on_device);
template <class C>
int prove_phase2_impl(pm_ctx *ctx, const uint64_t *x1, uint64_t *u_at_x1);
template <class C>
int prove_phase3_impl(pm_ctx *ctx, const uint64_t *x1, const uint64_t *x2, const uint64_t *a_at_x1,
                      const uint64_t *c_at_x1, uint64_t *d_xy, int *d_inf);

// prove_batch.hip: the three phases over a group of `rows` proofs against one unsharded key (blockIdx.y = proof).  x / w / r_a are `rows`
// records back to back.  Every phase only ENQUEUES on the context's stream: it reads its per-proof values from device memory and leaves
// its results there -- the (point, flag) records of [a]_1, [c]_1 (phase 1) and [d]_1 (phase 3) in pm_ctx::gw.pts, u(x1) of the rows in
// the array prove_batch_sums names, the flag word of proof b (prove.hip: k_check_sap) in pm_ctx::pb.flags[b].  Between them a glue
// provider writes the BatchRow records of pm_ctx::pb.rows (prove_batch_reserve sizes them): x1 before phase 2, the whole record before
// phase 3 -- the host (prove_batch_fetch1 / _fetch2 / _fetch3 synchronise and bring a phase's results down, prove_batch_rows2 / _rows3
// upload the records built from the host's challenges) or the kernels of prove_glue.hip (no copy, no synchronisation).
// prove_batch_group: the largest group the context's msm_max_piece and the HBM budget allow for `count` proofs; 0 = one proof's [d]_1
// row exceeds a piece (the caller loops over the per-proof path).
template <class C>
int prove_batch_group(pm_ctx *ctx, const pm_pk *pk, size_t count, size_t *group);
template <class C>
int prove_batch_reserve(pm_ctx *ctx, const pm_pk *pk, size_t rows);
template <class C>
int prove_batch_phase1(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *x, const uint64_t *w, bool assignment_on_device,
                       const uint64_t *r_a, bool xw_resident = false);
template <class C>
int prove_batch_phase2(pm_ctx *ctx, const pm_pk *pk, size_t rows);
template <class C>
int prove_batch_phase3(pm_ctx *ctx, const pm_pk *pk, size_t rows);
template <class C>
const Fp<typename C::FrP> *prove_batch_sums(pm_ctx *ctx, const pm_pk *pk, size_t rows);   // phase 2's u(x1), one per row (device)
template <class C>
int prove_batch_fetch1(pm_ctx *ctx, size_t rows, Affine<C> *a, int *a_inf, Affine<C> *c, int *c_inf, unsigned *flags_out);
template <class C>
int prove_batch_rows2(pm_ctx *ctx, size_t rows, const uint64_t *x1);
template <class C>
int prove_batch_fetch2(pm_ctx *ctx, const pm_pk *pk, size_t rows, uint64_t *u_at_x1);
template <class C>
int prove_batch_rows3(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *r_a, const uint64_t *x1, const uint64_t *x2, const uint64_t *a_at_x1,
                      const uint64_t *c_at_x1);
template <class C>
int prove_batch_fetch3(pm_ctx *ctx, size_t rows, Affine<C> *d, int *d_inf, unsigned *flags_out);

// prove_glue.hip: the device glue provider of pm_host_prove_batch (PM_PROVE_GLUE_DEVICE), one lane per proof.
//   glue_begin     once per call: tap 11 forgotten and sized for `count` proofs
//   glue_upload    per group, before phase 1: instance_host's rows and r_a go up (rows x m0 x 32 and rows x 64 bytes)
//   glue_x1        after phase 1: k_glue_x1 -- the records of [a]_1, [c]_1, the transcript, x1 into pb.rows; under `solve` the marker
//                  entries of the instance are replaced by the row's solved values and a stuck row is refused
//   glue_x2        after phase 2: k_glue_x2 -- a(x1), c(x1), x2, the whole phase-3 record into pb.rows, tap 11 of proofs g0 ...
//   glue_finish    after phase 3: k_proof_bytes, then the group's ONE copy to the host and ONE synchronisation; proofs / status are the
//                  group's first row's
// GPU ms of the three kernels go to T_POLY.
template <class C>
int glue_begin(pm_ctx *ctx, const pm_pk *pk, size_t count);
template <class C>
int glue_upload(pm_ctx *ctx, const pm_pk *pk, size_t rows, const uint64_t *instance_host, const uint64_t *r_a, size_t proof_len);
template <class C>
int glue_x1(pm_ctx *ctx, const pm_pk *pk, int transcript, size_t rows, bool solve);
template <class C>
int glue_x2(pm_ctx *ctx, const pm_pk *pk, int transcript, size_t rows, size_t g0);
template <class C>
int glue_finish(pm_ctx *ctx, const pm_pk *pk, size_t rows, bool solve, uint8_t *proofs, size_t proof_len, int *status);

// the group's [rows][m0 + mw] assignment buffer (pm_ctx::pb.xw), reserved: what prove_batch_phase1 reads with xw_resident
template <class C>
int prove_batch_xw(pm_ctx *ctx, const pm_pk *pk, size_t rows, Fp<typename C::FrP> **xw);

// solve.hip: PM_ASSIGNMENT_SOLVE.  A call with the flag runs, in this order:
//   solve_begin    forgets the last call's taps and sizes tap 9 for `count` assignments
//   solve_load     per group: the caller's x / w rows (host or device) -> rows of d_xw ([g][m0 + mw]), and the pattern kernel over them;
//                  g0 = index of the group's first assignment in the batch (assignment 0 sets the pattern)
//   solve_plan     after the last group: pattern and mismatch slot come down; PM_ERR_INVALID_ARG with pm_last_error set for a marker at
//                  column 0, a mismatching assignment or a structure that no row order solves; otherwise the plan is taken from the
//                  cache or built (pmsolve::build_plan_any_order: matrix order first, then the waiting-row scheduler)
//   solve_group    per group: the launch schedule over d_xw -- after a reordered plan k_solve_stuck_row, so that the stuck words hold
//                  rows for every reader, prove_glue.hip's kernels included --, then the stuck rows and completed instances of the
//                  group into tap 9; GPU ms go to timing_slot.  The stream is idle on return.
// solve_all is the four over a whole batch in groups of the check's size into pm_ctx::sv.xw ([count][m0 + mw], pm_prove_tap(10)).
template <class C>
int solve_begin(pm_ctx *ctx, const pm_pk *pk, size_t count);
template <class C>
int solve_load(pm_ctx *ctx, const pm_pk *pk, Fp<typename C::FrP> *d_xw, size_t g, size_t g0, const uint64_t *x, const uint64_t *w, bool on_device);
template <class C>
int solve_plan(pm_ctx *ctx, const pm_pk *pk);
template <class C>
int solve_group(pm_ctx *ctx, const pm_pk *pk, Fp<typename C::FrP> *d_xw, size_t g, size_t g0, int timing_slot);
template <class C>
int solve_all(pm_ctx *ctx, const pm_pk *pk, size_t count, const uint64_t *x, const uint64_t *w, bool on_device, size_t group, int timing_slot);
// the flag word of an `assignment_on_device` argument: false = a bit outside PM_ASSIGNMENT_DEVICE | PM_ASSIGNMENT_SOLVE
inline bool assignment_flags_ok(int f) { return (f & ~(PM_ASSIGNMENT_DEVICE | PM_ASSIGNMENT_SOLVE)) == 0; }
inline const uint64_t *solve_tap9_row(const pm_ctx *ctx, const pm_pk *pk, size_t i) { return ctx->sv.tap9.data() + i * 4 * (1 + pk->m0); }

template <class C>
int prove_phase1_sharded(pm_ctx *ctx, const pm_pk *pk, const uint64_t *x, const uint64_t *w, const uint64_t *r_a, uint64_t *a_xy, int *a_inf,
                         uint64_t *c_xy, int *c_inf, bool assignment_on_device);
template <class C>
int prove_phase2_sharded(pm_ctx *ctx, const uint64_t *x1, uint64_t *u_at_x1);
template <class C>
int prove_phase3_sharded(pm_ctx *ctx, const uint64_t *x1, const uint64_t *x2, const uint64_t *a_at_x1, const uint64_t *c_at_x1, uint64_t *d_xy,
                         int *d_inf);

// The helper context of `ctx` (own stream, own MSM workspace), created on first use with a copy of ctx's options; nullptr if it
// cannot be created (the callers then run their two jobs back to back).
inline pm_ctx *ctx_aux(pm_ctx *ctx) {
    if (!ctx->aux && pm_ctx_create(ctx->device, &ctx->aux) != PM_OK) ctx->aux = nullptr;
    if (ctx->aux) ctx->aux->opt = ctx->opt;
    return ctx->aux;
}

// The context's pinned host staging: [0, 4096) the asynchronous MSM's result slots (msm.hip) and phase 3's remainder, then
// PINNED_STAGE_BYTES for small device-to-host records that must land without stalling the host (prove_sharded.hip: phase 1's
// flags and halo coefficients -- a pageable destination makes hipMemcpyAsync wait for the stream).  nullptr on failure.
constexpr size_t PINNED_SLOTS_BYTES = 4096, PINNED_STAGE_BYTES = 32768;
constexpr size_t PINNED_MSM_SUM = 0,           // msm_begin -> msm_end: the reduced point of an enqueued MSM, internal form (XYZZ<C>)
                 PINNED_MSM_POINT = 1024,      // msm_begin -> msm_end: the affine result of an MSM that ran synchronously ...
                 PINNED_MSM_INF = 2048,        // ... and its infinity flag (int)
                 PINNED_REMAINDER = 3072,      // prove_sharded.hip, phase 3: the quotient's remainder H_0 (one Fr)
                 PINNED_FLAGS = PINNED_SLOTS_BYTES;   // the provers' status flags (4 bytes), first word of the staging area
template <class T>
inline T *pinned_slot(pm_ctx *ctx, size_t offset) { return (T *)((uint8_t *)ctx->h_pinned + offset); }
inline void *ctx_pinned(pm_ctx *ctx) {
    if (!ctx->h_pinned && hipHostMalloc(&ctx->h_pinned, PINNED_SLOTS_BYTES + PINNED_STAGE_BYTES, hipHostMallocDefault) != hipSuccess) ctx->h_pinned = nullptr;
    return ctx->h_pinned;
}

inline void timing_reset(pm_ctx *ctx) {
    for (int i = 0; i < T_NUM_SLOTS; ++i) ctx->timing_ms[i] = 0;
    // timers nobody asked for (lazy mode, below): their events go back to the pool unread -- the work they bracket finished with the
    // call that recorded them
    for (auto &t : ctx->pending_timers) { ctx->event_pool.push_back(t.a); ctx->event_pool.push_back(t.b); }
    ctx->pending_timers.clear();
}

// hipEvent stage timers (replace start_timer!/end_timer!, prover.rs:32-61).  Events are only
// recorded while a call runs; elapsed times are read in timing_flush() after the call's final
// stream synchronisation, so timing adds no host round trips.
struct StageTimer {
    pm_ctx *ctx;
    int slot;
    hipEvent_t a, b;
    bool ok;
    static bool take(pm_ctx *c, hipEvent_t *e) {
        if (!c->event_pool.empty()) { *e = c->event_pool.back(); c->event_pool.pop_back(); return true; }
        return hipEventCreate(e) == hipSuccess;
    }
    hipStream_t stream;
    StageTimer(pm_ctx *c, int s, hipStream_t on = nullptr) : ctx(c), slot(s), ok(false), stream(on ? on : c->stream) {
        if (!take(c, &a)) return;
        if (!take(c, &b)) { c->event_pool.push_back(a); return; }
        ok = hipEventRecord(a, stream) == hipSuccess;
        if (!ok) { c->event_pool.push_back(a); c->event_pool.push_back(b); }
    }
    void stop() {
        if (!ok) return;
        ok = false;
        (void)hipEventRecord(b, stream);
        ctx->pending_timers.push_back(PendingTimer{slot, a, b});
    }
    ~StageTimer() { stop(); }
};

// Reading ~18 event pairs costs ~40 us of host time per phase, with the GPU idle between the phases of a proof: pm_host_prove sets
// lazy_timings, the phases then leave their timers pending and pm_last_timings reads them when (if) somebody asks.
inline void timing_flush_now(pm_ctx *ctx) {
    for (auto &t : ctx->pending_timers) {
        float ms = 0;
        if (hipEventSynchronize(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess)
            ctx->timing_ms[t.slot] += ms;
        ctx->event_pool.push_back(t.a);
        ctx->event_pool.push_back(t.b);
    }
    ctx->pending_timers.clear();
}
inline void timing_flush(pm_ctx *ctx) {
    if (!ctx->lazy_timings) timing_flush_now(ctx);
}
// the helper context of the second MSM pipeline: reset / hand its stage times (or, lazily, its pending timers) to the owner
inline void timing_reset_aux(pm_ctx *ctx, pm_ctx *aux) {
    for (int i = 0; i < T_NUM_SLOTS; ++i) aux->timing_ms[i] = 0;   // its pending timers stay: the sharded prover's w transform ran on it
    aux->lazy_timings = ctx->lazy_timings;
}
inline void timing_absorb_aux(pm_ctx *ctx, pm_ctx *aux) {
    for (int s = 0; s < T_NUM_SLOTS; ++s) { ctx->timing_ms[s] += aux->timing_ms[s]; aux->timing_ms[s] = 0; }
    // lazy mode: the helper's unread timers (and their events) become the owner's; the helper's pool gets as many events back from the
    // owner's, or it would create new ones every proof while the owner's pool grows.  Called by the owner's thread, the helper idle.
    for (auto &t : aux->pending_timers) {
        ctx->pending_timers.push_back(t);
        for (int k = 0; k < 2 && !ctx->event_pool.empty(); ++k) { aux->event_pool.push_back(ctx->event_pool.back()); ctx->event_pool.pop_back(); }
    }
    aux->pending_timers.clear();
}

// Declared BEFORE a call's StageTimers: whatever path the call returns by (error statuses included), the stage timers
// that were started are read and their events destroyed -- stale entries would otherwise be added to the next
// proof's slots.
struct TimingGuard {
    pm_ctx *ctx;
    ~TimingGuard() { timing_flush(ctx); if (ctx->aux) timing_flush(ctx->aux); }
};

}  // namespace pm
