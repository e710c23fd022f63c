// C ABI of libpolymath_hip.so (include/polymath_hip.h): context / key management and dispatch
// on the curve.  All compute is in the .hip kernels; the host code here only moves buffers,
// and removes row-duplicate R1CS entries the reference cannot see (m_at, common.rs:100-105) when a matrix has any.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <thread>

#include <sys/random.h>

#include "internal.h"
#include "comm.h"
#include "fq28.cuh"
#include "prove_common.cuh"
#include "../host/hashes.hpp"
#include "../host/key_check.hpp"

using namespace pm;

extern "C" void pm_host_keccak_f1600(uint64_t state[25]) { pmhost::keccak_f1600(state); }

// ------------------------------------------------------------------------------ helpers
int pm::host_threads_env() {
    static const int env_threads = [] { const char *e = getenv("PM_HOST_THREADS"); return e ? std::max(1, atoi(e)) : 0; }();   // read once
    return env_threads;
}

// body(lo, hi, thread) over [0, count) in contiguous chunks on up to 32 host threads (one below 2^16 items).  An exception in a
// worker (bad_alloc) is caught there and re-thrown on the calling thread after the join -- never a std::terminate.
template <class F>
static void parallel_chunks(uint64_t count, F body) {
    unsigned T = std::thread::hardware_concurrency();
    if (T > 32) T = 32;
    if (T < 1 || count < ((uint64_t)1 << 16)) T = 1;
    const int env_threads = host_threads_env();
    if (env_threads) T = (unsigned)env_threads;
    if (T == 1) { body((uint64_t)0, count, 0u); return; }
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> errs(T);
    auto guarded_body = [&](uint64_t lo, uint64_t hi, unsigned t) {
        try { body(lo, hi, t); } catch (...) { errs[t] = std::current_exception(); }
    };
    for (unsigned t = 1; t < T; ++t) {
        try {
            th.emplace_back([=, &guarded_body] { guarded_body(count * t / T, count * (t + 1) / T, t); });
        } catch (const std::system_error &) {            // no more threads: this chunk runs here
            guarded_body(count * t / T, count * (t + 1) / T, t);
        }
    }
    guarded_body((uint64_t)0, count / T, 0u);
    for (auto &x : th) x.join();
    for (auto &e : errs)
        if (e) std::rethrow_exception(e);
}

template <class C>
static void repack_bases(const void *src, size_t stride, size_t len, Affine<C> *dst) {
    const size_t PT = sizeof(Affine<C>);
    const uint8_t *s = (const uint8_t *)src;
    for (size_t i = 0; i < len; ++i) {
        memcpy(&dst[i], s + i * stride, PT);
        if (stride > PT && s[i * stride + PT] != 0) dst[i] = Affine<C>::infinity();  // arkworks `infinity: bool`
    }
}

static int set_device(pm_ctx *ctx) {
    PM_HIP(ctx, hipSetDevice(ctx->device));
    return PM_OK;
}

// ------------------------------------------------------------------------------ context
extern "C" int pm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- options (include/polymath_hip.h: pm_option).  The environment gives a NEW context its defaults; it is read here, once per
// context, and nowhere on a proving path.
struct OptionSpec { const char *env; long long def, lo, hi; };
static const OptionSpec OPTION_SPECS[PM_NUM_OPTIONS] = {
    /* PM_OPT_MSM_OVERLAP       */ {"PM_MSM_OVERLAP", 1, 0, 1},
    /* PM_OPT_NTT_OVERLAP       */ {"PM_NTT_OVERLAP", 1, 0, 1},
    /* PM_OPT_TABLES            */ {"PM_TABLES", PM_TABLES_AUTO, PM_TABLES_OFF, PM_TABLES_NO_WIDE},
    /* PM_OPT_MSM_MAX_PIECE_LOG */ {"PM_MSM_MAX_PIECE_LOG", 27, 4, 27},
    /* PM_OPT_MAX_SEG_LOG       */ {"PM_MAX_SEG_LOG", 0, 0, 40},
    /* PM_OPT_INFLIGHT_CONTEXTS */ {"PM_INFLIGHT_CONTEXTS", 1, 1, 64},
    /* PM_OPT_MSM_TASK_LEN      */ {"PM_MSM_SEG", 0, 0, 1 << 20},
    /* PM_OPT_TABLE_WINDOW_BITS */ {"PM_TABLE_C", 0, 0, 532},     // accepted values: include/polymath_hip.h
    /* PM_OPT_WIRE_CHUNK_LOG    */ {"PM_WIRE_CHUNK_LOG", 20, 4, 24},
};
static void options_defaults(pm_options *o) {
    for (int k = 0; k < PM_NUM_OPTIONS; ++k) {
        long long v = OPTION_SPECS[k].def;
        if (const char *e = getenv(OPTION_SPECS[k].env)) {
            if (k == PM_OPT_TABLES) v = e[0] == 'w' ? PM_TABLES_WIDE : e[0] == '0' ? PM_TABLES_OFF : PM_TABLES_AUTO;   // 0 | 1 | wide
            else v = atoll(e);
            if (v < OPTION_SPECS[k].lo || v > OPTION_SPECS[k].hi) v = OPTION_SPECS[k].def;
        }
        o->v[k] = v;
    }
    if (o->v[PM_OPT_TABLES] == PM_TABLES_AUTO) {
        const char *e = getenv("PM_WIDE");
        if (e && e[0] == '0') o->v[PM_OPT_TABLES] = PM_TABLES_NO_WIDE;
    }
}

extern "C" int pm_ctx_set_option(pm_ctx *ctx, int option, long long value) {
    if (!ctx || option < 0 || option >= PM_NUM_OPTIONS) return PM_ERR_INVALID_ARG;
    if (value < OPTION_SPECS[option].lo || value > OPTION_SPECS[option].hi) return PM_ERR_INVALID_ARG;
    ctx->opt.v[option] = value;
    if (ctx->aux) ctx->aux->opt.v[option] = value;
    return PM_OK;
}
extern "C" int pm_ctx_get_option(const pm_ctx *ctx, int option, long long *value) {
    if (!ctx || !value || option < 0 || option >= PM_NUM_OPTIONS) return PM_ERR_INVALID_ARG;
    *value = ctx->opt.v[option];
    return PM_OK;
}

namespace pm {
uint64_t pk_serial_next() {
    static std::atomic<uint64_t> next{0};
    return ++next;
}
}  // namespace pm

extern "C" int pm_ctx_create(int device, pm_ctx **out) {
    if (!out) return PM_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PM_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return PM_ERR_INVALID_ARG;
    pm_ctx *ctx = new (std::nothrow) pm_ctx();
    if (!ctx) return PM_ERR_INVALID_ARG;
    ctx->device = device;
    options_defaults(&ctx->opt);
    ctx->pk = nullptr;
    ctx->phase = 0;
    ctx->aux = nullptr;
    ctx->comm = nullptr;
    ctx->tw_clock = 0;
    ctx->shard_roots_n = 0; ctx->shard_roots_N = 0; ctx->shard_roots_curve = -1;
    ctx->ntt_lds_attr[0] = ctx->ntt_lds_attr[1] = false;
    ctx->h_pinned = nullptr;
    ctx->msm_async = 0;
    ctx->keep_timings = false;
    ctx->lazy_timings = false;
    timing_reset(ctx);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return PM_ERR_HIP;
    }
    if (hipEventCreateWithFlags(&ctx->ev_sc_a, hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return PM_ERR_HIP;
    }
    *out = ctx;
    return PM_OK;
}

extern "C" void pm_ctx_destroy(pm_ctx *ctx) {
    if (!ctx) return;
    if (ctx->aux) pm_ctx_destroy(ctx->aux);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    timing_flush(ctx);
    MsmWorkspace &m = ctx->msm;
    for (DevBuf *b : {&m.set.sorted, &m.set.counts, &m.set.bucket_off, &m.set.task_off, &m.set.tasks, &m.set.partials, &m.set.task_cnt}) b->release();
    for (DevBuf *b : {&m.digits, &m.cursor, &m.wsum,
                      &m.region, &m.sub, &m.digits2, &m.len_bins, &m.block_cnt, &m.hot, &m.batch, &ctx->scratch, &ctx->sh_a, &ctx->sh_b, &ctx->sh_c, &ctx->halo,
                      &ctx->shard_roots, &ctx->ntt_tmp})
        b->release();
    ctx->pw.release();
    ctx->pb.release();
    ctx->sv.release();
    ctx->gw.release();
    for (auto &b : ctx->fb_table) b.release();
    for (auto &t : ctx->tw) { t.fwd.release(); t.inv.release(); t.fwd_int.release(); t.inv_int.release(); }
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    for (auto &t : ctx->pending_timers) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }   // pm_host_prove leaves them unread (lazy_timings)
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    (void)hipEventDestroy(ctx->ev_sc_a);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" const char *pm_last_error(const pm_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int pm_last_timings(pm_ctx *ctx, double *ms_out, int n_slots) {
    if (!ctx || !ms_out) return PM_ERR_INVALID_ARG;
    if (!ctx->pending_timers.empty()) {   // pm_host_prove leaves its stage timers unread (internal.h: lazy_timings)
        if (hipSetDevice(ctx->device) != hipSuccess) return PM_ERR_HIP;
        timing_flush_now(ctx);
    }
    for (int i = 0; i < n_slots; ++i) ms_out[i] = i < T_NUM_SLOTS ? ctx->timing_ms[i] : 0.0;
    return PM_OK;
}

// ---------------------------------------------------------------------------------- NTT
template <class C>
static int ntt_host(pm_ctx *ctx, uint64_t *data, unsigned log_n, int inverse) {
    typedef Fp<typename C::FrP> Fr;
    if (log_n > (unsigned)C::TWO_ADICITY) return PM_ERR_DOMAIN_TOO_LARGE;
    size_t bytes = sizeof(Fr) << log_n;
    PM_HIP(ctx, ctx->scratch.reserve(bytes));
    PM_HIP(ctx, hipMemcpyAsync(ctx->scratch.p, data, bytes, hipMemcpyHostToDevice, ctx->stream));
    timing_reset(ctx);
    PM_TRY(ntt_run<C>(ctx, ctx->scratch.as<Fr>(), log_n, inverse != 0));
    PM_HIP(ctx, hipMemcpyAsync(data, ctx->scratch.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    timing_flush(ctx);
    return PM_OK;
}

extern "C" int pm_ntt(pm_ctx *ctx, int curve, uint64_t *data, unsigned log_n, int inverse) {
    if (!ctx || !data) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return with_curve(curve, [&](auto cv) { return ntt_host<type_of<decltype(cv)>>(ctx, data, log_n, inverse); });
}

template <class C>
static int ntt_dev(pm_ctx *ctx, uint64_t *d, unsigned log_n, int inverse) {
    timing_reset(ctx);
    PM_TRY(ntt_run<C>(ctx, (Fp<typename C::FrP> *)d, log_n, inverse != 0));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    timing_flush(ctx);
    return PM_OK;
}

extern "C" int pm_ntt_device(pm_ctx *ctx, int curve, uint64_t *d_data, unsigned log_n, int inverse) {
    if (!ctx || !d_data) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return with_curve(curve, [&](auto cv) { return ntt_dev<type_of<decltype(cv)>>(ctx, d_data, log_n, inverse); });
}

template <class C>
static int ntt_batch_dev(pm_ctx *ctx, uint64_t *d, unsigned log_n, int inverse, size_t rows, size_t row_stride) {
    timing_reset(ctx);
    PM_TRY(ntt_run_batch<C>(ctx, (Fp<typename C::FrP> *)d, log_n, inverse != 0, rows, row_stride));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    timing_flush(ctx);
    return PM_OK;
}

extern "C" int pm_ntt_batch_device(pm_ctx *ctx, int curve, uint64_t *d_data, unsigned log_n, int inverse, size_t rows, size_t row_stride) {
    if (!ctx || !d_data) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return with_curve(curve, [&](auto cv) { return ntt_batch_dev<type_of<decltype(cv)>>(ctx, d_data, log_n, inverse, rows, row_stride); });
}

// ---------------------------------------------------------------------------------- MSM
struct BasesDeleter {   // frees the device allocations with the handle: error paths cannot leak HBM
    void operator()(pm_bases *b) const {
        if (!b) return;
        (void)hipSetDevice(b->device);
        if (b->d_points) (void)hipFree(b->d_points);
        if (b->d_inf) (void)hipFree(b->d_inf);
        if (b->d_table) (void)hipFree(b->d_table);
        delete b;
    }
};
typedef std::unique_ptr<pm_bases, BasesDeleter> BasesPtr;

template <class C>
static int bases_upload_impl(pm_ctx *ctx, const void *bases, size_t stride, size_t len, pm_bases **out) {
    if (stride < sizeof(Affine<C>)) return PM_ERR_INVALID_ARG;
    BasesPtr b(new pm_bases{C::ID, ctx->device, len, nullptr});
    if (len) {
        std::vector<Affine<C>> packed(len);
        repack_bases<C>(bases, stride, len, packed.data());
        PM_HIP(ctx, hipMalloc(&b->d_points, len * sizeof(Affine<C>)));
        PM_HIP(ctx, hipMemcpy(b->d_points, packed.data(), len * sizeof(Affine<C>), hipMemcpyHostToDevice));
        PM_TRY(bases_convert<C>(ctx, (Affine<C> *)b->d_points, len, true));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out = b.release();
    return PM_OK;
}

extern "C" int pm_bases_upload(pm_ctx *ctx, int curve, const void *bases, size_t base_stride, size_t len, pm_bases **out) {
    if (!ctx || !out || (len && !bases)) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return with_curve(curve, [&](auto cv) { return bases_upload_impl<type_of<decltype(cv)>>(ctx, bases, base_stride, len, out); });
}

template <class C>
static int bases_multiples_impl(pm_ctx *ctx, size_t len, pm_bases **out) {
    BasesPtr b(new pm_bases{C::ID, ctx->device, len, nullptr});
    if (len) {
        PM_HIP(ctx, hipMalloc(&b->d_points, len * sizeof(Affine<C>)));
        PM_TRY(bases_generate_multiples<C>(ctx, len, (Affine<C> *)b->d_points));
    }
    *out = b.release();
    return PM_OK;
}

extern "C" int pm_bases_generate_multiples(pm_ctx *ctx, int curve, size_t len, pm_bases **out) {
    if (!ctx || !out) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return with_curve(curve, [&](auto cv) { return bases_multiples_impl<type_of<decltype(cv)>>(ctx, len, out); });
}

// device -> host copy of resident (internal-form) points, converted back to standard Montgomery form
template <class C>
static int download_points(pm_ctx *ctx, const void *d_src, size_t len, uint64_t *out_xy) {
    if (!len) return PM_OK;
    PM_HIP(ctx, ctx->scratch.reserve(len * sizeof(Affine<C>)));
    PM_HIP(ctx, hipMemcpyAsync(ctx->scratch.p, d_src, len * sizeof(Affine<C>), hipMemcpyDeviceToDevice, ctx->stream));
    PM_TRY(bases_convert<C>(ctx, ctx->scratch.as<Affine<C>>(), len, false));
    PM_HIP(ctx, hipMemcpyAsync(out_xy, ctx->scratch.p, len * sizeof(Affine<C>), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PM_OK;
}

extern "C" int pm_bases_download(pm_ctx *ctx, const pm_bases *b, size_t offset, size_t len, uint64_t *out_xy) {
    if (!ctx || !b || !out_xy || offset + len > b->len) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    size_t pt = b->curve == PM_BLS12_381 ? sizeof(Affine<BlsCurve>) : sizeof(Affine<BnCurve>);
    const void *src = (const uint8_t *)b->d_points + offset * pt;
    return with_curve(b->curve, [&](auto cv) { return download_points<type_of<decltype(cv)>>(ctx, src, len, out_xy); });
}

template <class C>
static int bases_precompute_impl(pm_ctx *ctx, pm_bases *b) {
    if (b->tables.planned() || !b->len) return PM_OK;
    MsmTables tb(tables_plan(b->len, 1, b->len, (unsigned)C::FrP::BITS, decode_window_option((unsigned)ctx->opt.v[PM_OPT_TABLE_WINDOW_BITS])), b->len);
    if (!tb.planned()) return PM_OK;
    void *d_table = nullptr, *d_flags = nullptr;
    int st = PM_OK;
    if (hipMalloc(&d_table, b->len * tb.nwin * sizeof(TablePoint<C>)) != hipSuccess || hipMalloc(&d_flags, b->len) != hipSuccess) {
        ctx->err = "pm_bases_precompute: out of device memory for the window tables";
        st = PM_ERR_HIP;
    }
    if (st == PM_OK) st = infinity_flags<C>(ctx, (const Affine<C> *)b->d_points, b->len, (unsigned char *)d_flags);
    if (st == PM_OK) st = tables_build<C>(ctx, (const Affine<C> *)b->d_points, (TablePoint<C> *)d_table, b->len, tb);
    if (st != PM_OK) {
        if (d_table) (void)hipFree(d_table);
        if (d_flags) (void)hipFree(d_flags);
        return st;
    }
    b->d_table = d_table;
    b->d_inf = d_flags;
    tb.inf = (const unsigned char *)d_flags;
    tb.table = d_table;
    b->tables = tb;
    return PM_OK;
}

extern "C" int pm_bases_precompute(pm_ctx *ctx, pm_bases *b) {
    if (!ctx || !b) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return with_curve(b->curve, [&](auto cv) { return bases_precompute_impl<type_of<decltype(cv)>>(ctx, b); });
}

extern "C" size_t pm_bases_len(const pm_bases *b) { return b ? b->len : 0; }

extern "C" void pm_bases_free(pm_bases *b) { BasesDeleter()(b); }

template <class C>
static int msm_resident_impl(pm_ctx *ctx, const pm_bases *bases, size_t off, const uint64_t *scalars, int on_device,
                             size_t len, uint64_t *out_xy, int *out_inf) {
    typedef Fp<typename C::FrP> Fr;
    const Fr *d_sc = (const Fr *)scalars;
    if (!on_device && len) {
        PM_HIP(ctx, ctx->scratch.reserve(len * sizeof(Fr)));
        PM_HIP(ctx, hipMemcpyAsync(ctx->scratch.p, scalars, len * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        d_sc = ctx->scratch.as<Fr>();
    }
    Affine<C> r;
    int inf = 1;
    timing_reset(ctx);
    if (bases->tables.planned()) {
        MsmTables tb = bases->tables;
        tb.base_index = off;
        PM_TRY(msm_run<C>(ctx, (const Affine<C> *)nullptr, d_sc, len, &r, &inf, &tb));
    } else {
        PM_TRY(msm_run<C>(ctx, (const Affine<C> *)bases->d_points + off, d_sc, len, &r, &inf));
    }
    timing_flush(ctx);
    if (inf) memset(out_xy, 0, sizeof(Affine<C>));
    else memcpy(out_xy, &r, sizeof(Affine<C>));
    *out_inf = inf;
    return PM_OK;
}

extern "C" int pm_msm_g1_resident(pm_ctx *ctx, const pm_bases *bases, size_t base_offset, const uint64_t *scalars,
                                  int scalars_on_device, size_t len, uint64_t *out_xy, int *out_inf) {
    if (!ctx || !bases || !out_xy || !out_inf || (len && !scalars)) return PM_ERR_INVALID_ARG;
    if (base_offset + len > bases->len) return PM_ERR_LEN_MISMATCH;  // prover.rs:381
    PM_TRY(set_device(ctx));
    return with_curve(bases->curve, [&](auto cv) {
        return msm_resident_impl<type_of<decltype(cv)>>(ctx, bases, base_offset, scalars, scalars_on_device, len, out_xy, out_inf);
    });
}

template <class C>
static int msm_resident_batch_impl(pm_ctx *ctx, const pm_bases *bases, size_t off, const uint64_t *scalars, int on_device, size_t len,
                                   size_t batch, uint64_t *out_xy, int *out_inf) {
    typedef Fp<typename C::FrP> Fr;
    const Fr *d_sc = (const Fr *)scalars;
    if (!on_device && len) {
        PM_HIP(ctx, ctx->scratch.reserve(batch * len * sizeof(Fr)));
        PM_HIP(ctx, hipMemcpyAsync(ctx->scratch.p, scalars, batch * len * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        d_sc = ctx->scratch.as<Fr>();
    }
    std::vector<Affine<C>> r(batch);
    std::vector<int> inf(batch, 1);
    timing_reset(ctx);
    // the plain resident points, with or without window tables beside them (pm_bases_precompute keeps d_points)
    PM_TRY(msm_run_batch<C>(ctx, (const Affine<C> *)bases->d_points + off, d_sc, len, batch, r.data(), inf.data()));
    timing_flush(ctx);
    for (size_t b = 0; b < batch; ++b) {
        if (inf[b]) memset((uint8_t *)out_xy + b * sizeof(Affine<C>), 0, sizeof(Affine<C>));
        else memcpy((uint8_t *)out_xy + b * sizeof(Affine<C>), &r[b], sizeof(Affine<C>));
        out_inf[b] = inf[b];
    }
    return PM_OK;
}

extern "C" int pm_msm_g1_resident_batch(pm_ctx *ctx, const pm_bases *bases, size_t base_offset, const uint64_t *scalars,
                                        int scalars_on_device, size_t len, size_t batch, uint64_t *out_xy, int *out_inf) {
    if (batch == 1) return pm_msm_g1_resident(ctx, bases, base_offset, scalars, scalars_on_device, len, out_xy, out_inf);
    if (!ctx || !bases || (batch && (!out_xy || !out_inf || (len && !scalars)))) return PM_ERR_INVALID_ARG;
    if (base_offset + len > bases->len) return PM_ERR_LEN_MISMATCH;
    if (batch == 0) return PM_OK;
    PM_TRY(set_device(ctx));
    return with_curve(bases->curve, [&](auto cv) {
        return msm_resident_batch_impl<type_of<decltype(cv)>>(ctx, bases, base_offset, scalars, scalars_on_device, len, batch, out_xy, out_inf);
    });
}

extern "C" int pm_msm_g1(pm_ctx *ctx, int curve, const void *bases, size_t base_stride, const uint64_t *scalars,
                         size_t len, uint64_t *out_xy, int *out_inf) {
    if (!ctx || !out_xy || !out_inf || (len && (!bases || !scalars))) return PM_ERR_INVALID_ARG;
    pm_bases *b = nullptr;
    PM_TRY(pm_bases_upload(ctx, curve, bases, base_stride, len, &b));
    int st = pm_msm_g1_resident(ctx, b, 0, scalars, 0, len, out_xy, out_inf);
    pm_bases_free(b);
    return st;
}

template <class C>
static int g1_sum_impl(const uint64_t *pts, const int *infs, size_t count, uint64_t *out_xy, int *out_inf) {
    XYZZ<C> acc = XYZZ<C>::identity();
    for (size_t i = 0; i < count; ++i) {
        Affine<C> a;
        memcpy(&a, (const uint8_t *)pts + i * sizeof(Affine<C>), sizeof(Affine<C>));
        if (infs && infs[i]) continue;
        xyzz_madd<C>(acc, a, false);
    }
    Affine<C> r = xyzz_to_affine<C>(acc);
    int inf = acc.is_identity() ? 1 : 0;
    if (inf) memset(out_xy, 0, sizeof(Affine<C>));
    else memcpy(out_xy, &r, sizeof(Affine<C>));
    *out_inf = inf;
    return PM_OK;
}

extern "C" int pm_g1_sum(int curve, const uint64_t *points_xy, const int *infs, size_t count, uint64_t *out_xy, int *out_inf) {
    if (!out_xy || !out_inf || (count && !points_xy)) return PM_ERR_INVALID_ARG;
    return with_curve(curve, [&](auto cv) { return g1_sum_impl<type_of<decltype(cv)>>(points_xy, infs, count, out_xy, out_inf); });
}

// ------------------------------------------------------------------------- proving key
struct HostCsr {
    std::vector<uint64_t> rowptr;
    std::vector<uint32_t> col;
    std::vector<uint64_t> val;
};

// m_at (common.rs:100-105) only ever sees the FIRST entry of a row with a given column: the matrix without the later ones, its row
// pointers starting at 0.  The caller has checked rows and columns (pk_upload_matrices).
static void dedupe_csr(const pm_csr *m, uint64_t nr, HostCsr &out) {
    out.rowptr.assign(1, 0);
    for (uint64_t r = 0; r < nr; ++r) {
        const size_t start = out.col.size();
        for (uint64_t k = m->rowptr[r]; k < m->rowptr[r + 1]; ++k) {
            if (std::find(out.col.begin() + start, out.col.end(), m->col[k]) != out.col.end()) continue;
            out.col.push_back(m->col[k]);
            out.val.insert(out.val.end(), m->val + 4 * k, m->val + 4 * k + 4);
        }
        out.rowptr.push_back(out.col.size());
    }
}

extern "C" void pm_pk_free(pm_pk *pk) { delete pk; }   // the key owns its device memory (internal.h)

template <class C>
static int pk_upload_matrices(pm_ctx *ctx, pm_pk *pk, const pm_csr *a, const pm_csr *b, const pm_csr *c) {
    const pm_csr *m[3] = {a, b, c};
    const uint64_t nr = pk->nr, ncols = pk->m0 + pk->mw;
    for (int i = 0; i < 3; ++i) {
        if (!m[i] || m[i]->nrows != nr || !m[i]->rowptr) return PM_ERR_INVALID_ARG;
        // The one check of a matrix, one parallel pass over its rows: row pointers, column range, and whether ANY row repeats a
        // column (m_at, common.rs:100-105, only ever sees the first entry).  Without repeats -- every circuit ark-relations'
        // `to_matrices` produces after its own linear-combination merging, and the synthetic ones -- the caller's arrays go to the
        // device as they are: no host copy (round 4: the copying first-entry pass was 1.05 s of host time at 2^24 gates).
        std::atomic<int> bad{0}, repeats{0};
        const pm_csr *mi = m[i];
        parallel_chunks(nr, [&](uint64_t lo, uint64_t hi, unsigned) {
            for (uint64_t r = lo; r < hi; ++r) {
                const uint64_t k0 = mi->rowptr[r], k1 = mi->rowptr[r + 1];
                if (k1 < k0) { bad = 1; return; }
                for (uint64_t k = k0; k < k1; ++k) {
                    if (mi->col[k] >= ncols) { bad = 1; return; }
                    for (uint64_t q = k0; q < k; ++q)
                        if (mi->col[q] == mi->col[k]) { repeats = 1; break; }
                }
            }
        });
        if (bad) return PM_ERR_INVALID_ARG;
        HostCsr h;
        const uint64_t *rowptr = mi->rowptr, *val = mi->val;
        const uint32_t *col = mi->col;
        uint64_t nnz = nr ? mi->rowptr[nr] - mi->rowptr[0] : 0;
        if (repeats || (nr && mi->rowptr[0] != 0)) {
            dedupe_csr(mi, nr, h);
            rowptr = h.rowptr.data(); col = h.col.data(); val = h.val.data();
            nnz = h.col.size();
        }
        const uint64_t zero_row = 0;
        pk->nnz[i] = nnz;
        PM_HIP(ctx, pk->alloc(&pk->d_rowptr[i], (nr + 1) * 8));
        PM_HIP(ctx, hipMemcpy(pk->d_rowptr[i], nr ? rowptr : &zero_row, (nr + 1) * 8, hipMemcpyHostToDevice));
        const size_t nz = nnz ? nnz : 1;
        PM_HIP(ctx, pk->alloc(&pk->d_col[i], nz * 4));
        PM_HIP(ctx, pk->alloc(&pk->d_val[i], nz * 32));
        if (nnz) {
            PM_HIP(ctx, hipMemcpy(pk->d_col[i], col, nnz * 4, hipMemcpyHostToDevice));
            PM_HIP(ctx, hipMemcpy(pk->d_val[i], val, nnz * 32, hipMemcpyHostToDevice));
        }
    }
    return PM_OK;
}

// Apply `fill(vec, start, count, dst)` to every piece of the logical concatenation range [lo, hi).
template <class C, class F>
static int for_cat_range(const pm_pk *pk, uint64_t lo, uint64_t hi, Affine<C> *dst, F fill) {
    for (int v : pmlayout::CAT_ORDER) {
        uint64_t s = pk->seg_off[v], e = s + pk->base_len[v];
        uint64_t a = std::max(lo, s), b = std::min(hi, e);
        if (a >= b) continue;
        PM_TRY(fill(v, a - s, b - a, dst + (a - lo)));
    }
    return PM_OK;
}

// Sized for 288 GB of HBM: window tables for the merged MSMs that table_grants (key_plan.hpp) gives them to, the infinity flags of the
// wide mode for those it gives that.
template <class C>
static int pk_build_tables(pm_ctx *ctx, pm_pk *pk) {
    pk->max_piece = (uint64_t)msm_max_piece(ctx);
    size_t free_b = 0, total_b = 0;
    PM_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t vec_n = pk->layout == PM_SHARD_VECTOR ? pk->n / (uint64_t)pk->shard_count : pk->n;   // length of a rank's vectors
    const auto grants = table_grants(free_b, (int)ctx->opt.v[PM_OPT_INFLIGHT_CONTEXTS], vec_n, pk->res_cnt, pk->max_piece, ctx->opt.v[PM_OPT_TABLES],
                                     (unsigned)ctx->opt.v[PM_OPT_TABLE_WINDOW_BITS], (unsigned)C::FrP::BITS, sizeof(TablePoint<C>));
    for (int k = 0; k < 3; ++k) {
        if (grants[k].kind == Grant::NONE) continue;
        const bool wide = grants[k].kind == Grant::WIDE;
        const size_t len = (size_t)pk->res_cnt[k];
        const Affine<C> *points = (const Affine<C> *)pk->d_bases + pk->res_dev_off[k];
        MsmTables tb(grants[k].layout, wide ? 0 : len);
        if (!wide) PM_HIP(ctx, pk->alloc(&pk->d_tab[k], len * tb.nwin * sizeof(TablePoint<C>)));
        PM_HIP(ctx, pk->alloc(&pk->d_tab_inf[k], len));
        PM_TRY(infinity_flags<C>(ctx, points, len, (unsigned char *)pk->d_tab_inf[k]));
        if (!wide) PM_TRY(tables_build<C>(ctx, points, (TablePoint<C> *)pk->d_tab[k], len, tb));
        tb.inf = (const unsigned char *)pk->d_tab_inf[k];
        tb.table = pk->d_tab[k];
        pk->tables[k] = tb;
    }
    return PM_OK;
}

// The one skeleton of the three ways a key comes to be (pm_pk_load*, pm_pk_load_bytes, pm_pk_generate*): plan, segment lists, matrices,
// resident points, window tables.  *out is written on success only; on every other way out the key goes, and its device memory with it.
//   planned(st, pk)   after key_plan, with its status: the caller's own checks of the shape; returns the status to go on with
//   uploaded(st, pk)  after pk_upload_matrices, likewise: what the caller prepares once the matrices are resident
//   fill(vec, start, count, dst)   points [start, start + count) of base vector `vec` to the device at dst, in the internal form
//   filled(pk)        between the fill and the tables: the byte loader reads its verdicts, frees its staging -- the tables want the
//                     memory -- and, asked to, checks the key's relations on the plain resident points (key_check.hip)
template <class C, class Planned, class Uploaded, class Fill, class Filled>
static int pk_build(pm_ctx *ctx, uint64_t m0, uint64_t mw, uint64_t nr, int shard_rank, int shard_count, int layout, const pm_csr *a, const pm_csr *b,
                    const pm_csr *c, Planned planned, Uploaded uploaded, Fill fill, Filled filled, pm_pk **out) {
    typedef typename C::FrP P;
    std::unique_ptr<pm_pk> pk(new pm_pk());
    pk->curve = C::ID;
    pk->device = ctx->device;
    const long long seg_log = ctx->opt.v[PM_OPT_MAX_SEG_LOG];   // test knob: many tiny sub-segments
    const int st = key_plan(C::TWO_ADICITY, m0, mw, nr, shard_rank, shard_count, layout, seg_log > 0 ? (uint64_t)1 << seg_log : 0, *pk);
    Fp<P> w;   // omega: the generator of the size-n domain
    for (int i = 0; i < P::N; ++i) w.l[i] = C::ROOT_MONT[i];
    for (unsigned i = pk->log_n; i < (unsigned)C::TWO_ADICITY; ++i) w = sqr<P>(w);
    memcpy(pk->omega, w.l, 32);
    PM_TRY(planned(st, *pk));
    if (pk->layout == PM_SHARD_VECTOR) {   // the division scan reads both lists on the device (prove_sharded.hip: k_seg_base, k_seg_chain)
        PM_HIP(ctx, pk->alloc(&pk->d_segs, pk->segs.size() * sizeof(pmlayout::Segment)));
        PM_HIP(ctx, hipMemcpy(pk->d_segs, pk->segs.data(), pk->segs.size() * sizeof(pmlayout::Segment), hipMemcpyHostToDevice));
        PM_HIP(ctx, pk->alloc(&pk->d_all_segs, pk->all_segs.size() * sizeof(pm_pk::SegRef)));
        PM_HIP(ctx, hipMemcpy(pk->d_all_segs, pk->all_segs.data(), pk->all_segs.size() * sizeof(pm_pk::SegRef), hipMemcpyHostToDevice));
    }
    PM_TRY(uploaded(pk_upload_matrices<C>(ctx, pk.get(), a, b, c), *pk));
    PM_HIP(ctx, pk->alloc(&pk->d_bases, std::max<uint64_t>(pk->resident_points(), 1) * sizeof(Affine<C>)));
    PM_TRY(pk->for_resident([&](uint64_t lo, uint64_t count, uint64_t at) {
        return count ? for_cat_range<C>(pk.get(), lo, lo + count, (Affine<C> *)pk->d_bases + at, fill) : (int)PM_OK;
    }));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PM_TRY(filled(*pk));
    PM_TRY(pk_build_tables<C>(ctx, pk.get()));
    *out = pk.release();
    return PM_OK;
}
static int pk_pass(int st, const pm_pk &) { return st; }   // a caller of pk_build with nothing to do at a step
static int pk_nothing(const pm_pk &) { return PM_OK; }

// The way in of all three: the device, the curve, and a host exception while the key is read or built (bad_alloc in the parse of the
// bytes, in a matrix copy, in the plan's vectors) as a status with the message in pm_last_error, never an abort.
template <class F>
static int pk_entry(pm_ctx *ctx, int curve, F body) {
    PM_TRY(set_device(ctx));
    try {
        return with_curve(curve, body);
    } catch (const std::exception &e) {
        ctx->err = e.what();
        return PM_ERR_STATE;
    }
}

template <class C>
static int pk_load_impl(pm_ctx *ctx, uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t sigma, const pm_csr *a,
                        const pm_csr *b, const pm_csr *c, const pm_base_array *bases, int shard_rank, int shard_count, int layout,
                        pm_pk **out) {
    std::vector<Affine<C>> tmp;
    return pk_build<C>(
        ctx, m0, mw, nr, shard_rank, shard_count, layout, a, b, c,
        [&](int st, const pm_pk &pk) -> int {
            if (st) return st;
            if (pk.n != n || pk.sigma != sigma) return PM_ERR_INVALID_ARG;
            for (int v = 0; v < PM_NUM_BASE_VECS; ++v)
                if (bases[v].len < pk.base_len[v] || bases[v].stride < sizeof(Affine<C>) || !bases[v].points) return PM_ERR_LEN_MISMATCH;
            return PM_OK;
        },
        pk_pass,
        [&](int v, uint64_t start, uint64_t count, Affine<C> *dst) -> int {
            tmp.resize(count);
            repack_bases<C>((const uint8_t *)bases[v].points + start * bases[v].stride, bases[v].stride, count, tmp.data());
            PM_HIP(ctx, hipMemcpy(dst, tmp.data(), count * sizeof(Affine<C>), hipMemcpyHostToDevice));
            PM_TRY(bases_convert<C>(ctx, dst, count, true));
            PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
            return PM_OK;
        },
        pk_nothing, out);
}

extern "C" int pm_pk_load_sharded(pm_ctx *ctx, int curve, uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t sigma,
                                  const pm_csr *a, const pm_csr *b, const pm_csr *c, const pm_base_array bases[PM_NUM_BASE_VECS],
                                  int shard_rank, int shard_count, int layout, pm_pk **out) {
    if (!ctx || !a || !b || !c || !bases || !out) return PM_ERR_INVALID_ARG;
    return pk_entry(ctx, curve, [&](auto cv) {
        return pk_load_impl<type_of<decltype(cv)>>(ctx, n, m0, mw, nr, sigma, a, b, c, bases, shard_rank, shard_count, layout, out);
    });
}

extern "C" int pm_pk_load(pm_ctx *ctx, int curve, uint64_t n, uint64_t m0, uint64_t mw, uint64_t nr, uint64_t sigma,
                          const pm_csr *a, const pm_csr *b, const pm_csr *c, const pm_base_array bases[PM_NUM_BASE_VECS],
                          int shard_rank, int shard_count, pm_pk **out) {
    return pm_pk_load_sharded(ctx, curve, n, m0, mw, nr, sigma, a, b, c, bases, shard_rank, shard_count, PM_SHARD_PAIRS, out);
}

// ---- keys as bytes (ProvingKey::serialize_compressed; g1_codec.hip decodes the points)
static const char *const *const BASE_VEC_NAMES = pmhost::KEY_VEC_NAMES;   // host/key_check.hpp: the relation texts name the same vectors
static const int WIRE_VECTOR_ORDER[PM_NUM_BASE_VECS] = {PM_X_POWERS, PM_X_POWERS_Y_ALPHA, PM_X_POWERS_ZH_BY_Y_ALPHA, PM_X_POWERS_Y_GAMMA,
                                                        PM_X_POWERS_Y_GAMMA_Z, PM_UJ_WJ_LCS_BY_Y_ALPHA};   // data_structures.rs:60-72

static size_t wire_chunk(const pm_ctx *ctx) { return (size_t)1 << ctx->opt.v[PM_OPT_WIRE_CHUNK_LOG]; }

struct PinnedPair {   // two pinned staging buffers, freed with the call
    void *p[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~PinnedPair() {
        for (int k = 0; k < 2; ++k) {
            if (ev[k]) (void)hipEventDestroy(ev[k]);
            if (p[k]) (void)hipHostFree(p[k]);
        }
    }
};

template <class C>
static int pk_load_bytes_impl(pm_ctx *ctx, const uint8_t *bytes, size_t len, int validate, int shard_rank, int shard_count, int layout,
                              pm_pk **out) {
    const int form = validate & PM_WIRE_UNCOMPRESSED;   // bit 8 selects the record form; validation is every other bit
    validate &= ~PM_WIRE_UNCOMPRESSED;
    const bool relations = (validate & PM_KEY_CHECK_RELATIONS) != 0;   // one of those other bits: the relation check implies validation
    const size_t NB = g1_record_bytes<C>(form);
    auto fail = [&](int st, const std::string &why) { if (!why.empty()) ctx->err = "pm_pk_load_bytes: " + why; return st; };
    if (relations && (shard_count != 1 || layout != PM_SHARD_PAIRS))
        return fail(PM_ERR_INVALID_ARG, "PM_KEY_CHECK_RELATIONS needs the whole key on one device: shard_count 1, PM_SHARD_PAIRS");
    WireLayout w;
    PM_TRY(pk_wire_parse<C>(bytes, len, form, w, ctx->err));
    pm_csr m[3];
    for (int k = 0; k < 3; ++k) {
        if (w.col[k].empty()) { w.col[k].push_back(0); w.val[k].assign(4, 0); }   // non-null pointers for an empty matrix
        m[k] = pm_csr{w.nr, w.rowptr[k].data(), w.col[k].data(), w.val[k].data()};
    }
    // The point records of each requested range go through two staging slots (chunk x record size bytes each), each a pinned host buffer and a device buffer:
    // the host copies chunk k + 1 out of the caller's bytes (an mmap, say) while the device decodes chunk k.  A slot is refilled
    // only after the decode that read it has finished (its event is recorded behind the kernel), whatever way the runtime moves
    // the copy.  Refused points lower a per-vector slot; nothing is read back until the whole resident set is decoded.
    const size_t CH = wire_chunk(ctx);
    ScopedDevBuf d_in[2], d_bad;
    PinnedPair pin;
    int slot = 0;
    bool used[2] = {false, false};
    return pk_build<C>(
        ctx, w.m0, w.mw, w.nr, shard_rank, shard_count, layout, &m[0], &m[1], &m[2],
        [&](int st, const pm_pk &pk) -> int {
            if (st) return fail(st, "the key's shape or the shard arguments are not supported");
            // the checks of pmhost::pk_load: the prover hashes the vk's n / m0 / omega while the device derives its own from the SAP header
            if (w.vk_m0 != w.m0) return fail(PM_ERR_INVALID_ARG, "vk.m0 disagrees with the SAP matrices' m0");
            if (w.n != pk.n || w.sigma != pk.sigma) return fail(PM_ERR_INVALID_ARG, "vk.n / vk.sigma disagree with the domain of the SAP matrices");
            if (memcmp(w.omega, pk.omega, 32) != 0) return fail(PM_ERR_INVALID_ARG, "vk.omega is not the generator of the size-n domain");
            for (int v = 0; v < PM_NUM_BASE_VECS; ++v)
                if (w.vec_len[v] != pk.base_len[v])
                    return fail(PM_ERR_INVALID_ARG, std::string(BASE_VEC_NAMES[v]) + ": length " + std::to_string(w.vec_len[v]) +
                                                        " does not match the key's shape (" + std::to_string(pk.base_len[v]) + ")");
            for (int k = 0; k < 3; ++k)
                if (w.rowptr[k].size() != w.nr + 1) return fail(PM_ERR_INVALID_ARG, "a matrix does not have num_constraints rows");
            return PM_OK;
        },
        [&](int st, const pm_pk &) -> int {
            if (st) return fail(st, st == PM_ERR_HIP ? "" : "a matrix column is out of range");
            if (d_in[0].reserve(CH * NB) != hipSuccess || d_in[1].reserve(CH * NB) != hipSuccess || d_bad.reserve(PM_NUM_BASE_VECS * 8) != hipSuccess)
                return fail(PM_ERR_HIP, "out of device memory for the staging buffers");
            for (int k = 0; k < 2; ++k)
                if (hipHostMalloc(&pin.p[k], CH * NB, hipHostMallocDefault) != hipSuccess ||
                    hipEventCreateWithFlags(&pin.ev[k], hipEventDisableTiming) != hipSuccess)
                    return fail(PM_ERR_HIP, "out of pinned host memory for the staging buffers");
            if (hipMemsetAsync(d_bad.p, 0xFF, PM_NUM_BASE_VECS * 8, ctx->stream) != hipSuccess) return fail(PM_ERR_HIP, "hipMemsetAsync failed");
            return PM_OK;
        },
        [&](int v, uint64_t start, uint64_t count, Affine<C> *dst) -> int {
            for (uint64_t s = 0; s < count; s += CH) {
                const uint64_t cnt = std::min<uint64_t>(CH, count - s);
                if (used[slot]) PM_HIP(ctx, hipEventSynchronize(pin.ev[slot]));
                memcpy(pin.p[slot], bytes + w.vec_off[v] + (start + s) * NB, cnt * NB);
                PM_HIP(ctx, hipMemcpyAsync(d_in[slot].p, pin.p[slot], cnt * NB, hipMemcpyHostToDevice, ctx->stream));
                PM_TRY(g1_decode_device<C>(ctx, d_in[slot].as<uint8_t>(), cnt, validate != 0, dst + s, nullptr, d_bad.as<unsigned long long>() + v, start + s, form));
                PM_HIP(ctx, hipEventRecord(pin.ev[slot], ctx->stream));
                used[slot] = true;
                slot ^= 1;
                PM_TRY(bases_convert<C>(ctx, dst + s, cnt, true));
            }
            return PM_OK;
        },
        [&](const pm_pk &pk) -> int {
            unsigned long long h_bad[PM_NUM_BASE_VECS];
            if (hipMemcpy(h_bad, d_bad.p, sizeof(h_bad), hipMemcpyDeviceToHost) != hipSuccess) return fail(PM_ERR_HIP, "reading the verdicts failed");
            for (int v : WIRE_VECTOR_ORDER)
                if (h_bad[v] != ~0ull)
                    return fail(PM_ERR_INVALID_ARG, std::string(BASE_VEC_NAMES[v]) + "[" + std::to_string(h_bad[v] >> 8) + "]: " +
                                                        g1_status_text(C::ID, (int)(h_bad[v] & 0xFF), form));
            for (ScopedDevBuf &b : d_in) b.release();   // before the tables: they want the memory
            if (!relations) return PM_OK;
            // The loader is the verifier of this check and the key's bytes are fixed by now: the weights' seed comes from the operating
            // system, per call, and a load that gets none is refused.
            if (w.vk_g2_inf) return fail(PM_ERR_INVALID_ARG, "a G2 point of the vk is the point at infinity");
            uint8_t seed[32];
            for (size_t got = 0; got < sizeof seed;) {
                const ssize_t r = getrandom(seed + got, sizeof seed - got, 0);
                if (r <= 0) return fail(PM_ERR_STATE, "no random bytes from the operating system for the relation check");
                got += (size_t)r;
            }
            Affine<C> one_g1;
            memcpy((void *)&one_g1, w.vk_one_g1, sizeof one_g1);
            int failed = pmhost::KEY_REL_NONE;
            PM_TRY(key_check_run<C>(ctx, &pk, one_g1, w.vk_g2, seed, &failed));
            if (failed != pmhost::KEY_REL_NONE) return fail(PM_ERR_INVALID_ARG, pmhost::key_relation_text(failed));
            return PM_OK;
        },
        out);
}

static int pm_pk_set_hints(pm_ctx *ctx, pm_pk *pk, const uint64_t *desc, size_t n_words);

extern "C" int pm_pk_load_bytes(pm_ctx *ctx, int curve, const uint8_t *bytes, size_t len, int validate, int shard_rank, int shard_count,
                                int layout, pm_pk **out) {
    if (validate & PM_KEY_HINTS) {   // no key is loaded: `bytes` declares the hints of the existing key *out, which stays where it is
        if (!ctx || !out || !*out || (len && !bytes)) return PM_ERR_INVALID_ARG;
        if (validate != PM_KEY_HINTS || (*out)->curve != curve || len % sizeof(uint64_t) != 0) {
            ctx->err = "pm_pk_load_bytes: PM_KEY_HINTS stands alone in `validate`, takes the key's curve and a whole number of 64-bit words";
            return PM_ERR_INVALID_ARG;
        }
        std::vector<uint64_t> desc(len / sizeof(uint64_t));   // the caller's bytes need not be aligned
        if (len) memcpy(desc.data(), bytes, len);
        return pm_pk_set_hints(ctx, *out, desc.data(), desc.size());
    }
    if (!ctx || !bytes || !out) return PM_ERR_INVALID_ARG;
    *out = nullptr;
    return pk_entry(ctx, curve, [&](auto cv) {
        return pk_load_bytes_impl<type_of<decltype(cv)>>(ctx, bytes, len, validate, shard_rank, shard_count, layout, out);
    });
}

template <class C>
static int g1_decode_impl(pm_ctx *ctx, const uint8_t *in, size_t count, int validate, uint64_t *out_xy, uint8_t *status) {
    const int form = validate & PM_WIRE_UNCOMPRESSED;
    validate &= ~PM_WIRE_UNCOMPRESSED;
    const size_t NB = g1_record_bytes<C>(form), CH = wire_chunk(ctx);
    ScopedDevBuf d_in, d_out, d_st;
    const size_t first = std::min(count, CH);
    PM_HIP(ctx, d_in.reserve(first * NB));
    PM_HIP(ctx, d_out.reserve(first * sizeof(Affine<C>)));
    PM_HIP(ctx, d_st.reserve(first));
    for (size_t s = 0; s < count; s += CH) {
        const size_t cnt = std::min(CH, count - s);
        PM_HIP(ctx, hipMemcpyAsync(d_in.p, in + s * NB, cnt * NB, hipMemcpyHostToDevice, ctx->stream));
        PM_TRY(g1_decode_device<C>(ctx, d_in.as<uint8_t>(), cnt, validate != 0, d_out.as<Affine<C>>(), d_st.as<uint8_t>(), nullptr, 0, form));
        PM_HIP(ctx, hipMemcpyAsync((uint8_t *)out_xy + s * sizeof(Affine<C>), d_out.p, cnt * sizeof(Affine<C>), hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipMemcpyAsync(status + s, d_st.p, cnt, hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PM_OK;
}

extern "C" int pm_g1_decode(pm_ctx *ctx, int curve, const uint8_t *in, size_t count, int validate, uint64_t *out_xy, uint8_t *status) {
    if (!ctx || (count && (!in || !out_xy || !status))) return PM_ERR_INVALID_ARG;
    if (!count) return PM_OK;
    PM_TRY(set_device(ctx));
    return with_curve(curve, [&](auto cv) { return g1_decode_impl<type_of<decltype(cv)>>(ctx, in, count, validate, out_xy, status); });
}

// generate_proving_key (generator.rs:24-167) with the trapdoors supplied.  The dense uj_wj_lcs loop
// (:112-136) becomes one sparse pass over A, B, C:
//   column j' of z_tail (j = j' + m0), L1 = L[2m0+r], L2 = L[2m0+nr+r]:
//     R1CS column k = j' < m0+mw:  u = sum_r A[r][k](L1+L2) + B[r][k](L1-L2)
//                                  w = 4 sum_r C[r][k] L1  (+ 4 L[k] if k < m0)
//     y column t = j' - (m0+mw):   u = 0, w = L[t] + L[t+m0] (t < m0) | L1 + L2 (t = m0 + r)
template <class C>
static int pk_generate_impl(pm_ctx *ctx, uint64_t m0, uint64_t mw, uint64_t nr, const pm_csr *a, const pm_csr *b,
                            const pm_csr *c, const uint64_t *x_trap, const uint64_t *z_trap, int shard_rank,
                            int shard_count, int layout, pm_pk **out) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    HostProfile hp("setup", shard_rank);            // PM_PROFILE_HOST=1: where the host thread's time goes (stderr)
    Fr x, z;
    memcpy(x.l, x_trap, 32);
    memcpy(z.l, z_trap, 32);
    Fr scale[PM_NUM_BASE_VECS];                     // per-vector scale of the x-power vectors (generator.rs:82-109)
    ScopedDevBuf d_lcs_buf;
    const uint64_t CH = (uint64_t)1 << 22;
    const int st = pk_build<C>(
        ctx, m0, mw, nr, shard_rank, shard_count, layout, a, b, c,
        [&](int st, const pm_pk &) { hp.mark("layout"); return st; },
        [&](int st, const pm_pk &pk) -> int {
            if (st) return st;
            hp.mark("matrices: first-entry pass + upload");
            const uint64_t n = pk.n, Lz = pk.base_len[PM_UJ_WJ_LCS_BY_Y_ALPHA];
            Fr omega;
            memcpy(omega.l, pk.omega, 32);
            Fr xn = pow_u64<P>(x, n), one = Fr::one();
            if (xn.eq(one) || pow_u64<P>(z, n).eq(one)) return PM_ERR_INVALID_ARG;          // sample_element_outside_domain
            Fr y = pow_u64<P>(x, pk.sigma), yinv = inverse<P>(y);                           // generator.rs:73
            Fr y_alpha = pow_u64<P>(yinv, 3), y_to_minus_alpha = pow_u64<P>(y, 3), y_gamma = pow_u64<P>(yinv, 5);
            Fr zh = sub<P>(xn, one);                                                        // :106
            // uj_wj_lcs scalars (generator.rs:112-136) on the device: Lagrange coefficients at x by chunked batch inversion, the sparse
            // pass over the CSR matrices uploaded just now (setup.hip: lcs_scalars).  Rounds 1-3 ran both on <= 32 host threads.
            ScopedDevBuf d_lagrange, d_work;
            if (hipMalloc(&d_lcs_buf.p, (Lz ? Lz : 1) * sizeof(Fr)) != hipSuccess) { ctx->err = "out of device memory for the lcs scalars"; return PM_ERR_HIP; }
            d_lcs_buf.bytes = (Lz ? Lz : 1) * sizeof(Fr);
            const Fr kscale = mul<P>(zh, inverse<P>(from_u64<P>(n)));
            PM_TRY(lcs_scalars<C>(ctx, &pk, x, omega, kscale, y_gamma, y_to_minus_alpha, d_lagrange, d_work, d_lcs_buf.as<Fr>()));
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "lcs scalars: stream failed"; return PM_ERR_HIP; }
            hp.mark("lcs scalars (device, synchronised)");
            scale[PM_X_POWERS] = one;
            scale[PM_X_POWERS_Y_ALPHA] = y_alpha;
            scale[PM_X_POWERS_Y_GAMMA] = y_gamma;
            scale[PM_X_POWERS_Y_GAMMA_Z] = mul<P>(y_gamma, z);
            scale[PM_X_POWERS_ZH_BY_Y_ALPHA] = mul<P>(zh, y_to_minus_alpha);
            return PM_OK;
        },
        [&](int v, uint64_t start, uint64_t count, Affine<C> *dst) -> int {
            PM_HIP(ctx, ctx->scratch.reserve(std::min(count, CH) * sizeof(Fr)));
            Fr *d_sc = ctx->scratch.as<Fr>();
            for (uint64_t s = 0; s < count; s += CH) {
                uint64_t cnt = std::min(CH, count - s);
                const Fr *src = d_sc;
                if (v == PM_UJ_WJ_LCS_BY_Y_ALPHA) {
                    src = d_lcs_buf.as<Fr>() + start + s;
                } else {
                    Fr first = mul<P>(scale[v], pow_u64<P>(x, start + s));
                    PM_TRY(powers_fill<C>(ctx, d_sc, cnt, first, x));
                }
                PM_TRY(fixed_base_batch<C>(ctx, src, cnt, dst + s));
                PM_TRY(bases_convert<C>(ctx, dst + s, cnt, true));
                PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            return PM_OK;
        },
        pk_nothing, out);
    if (st == PM_OK) hp.mark("bases + tables (device, synchronised)");
    return st;
}

extern "C" int pm_pk_generate_sharded(pm_ctx *ctx, int curve, uint64_t m0, uint64_t mw, uint64_t nr, const pm_csr *a,
                                      const pm_csr *b, const pm_csr *c, const uint64_t *x_trapdoor, const uint64_t *z_trapdoor,
                                      int shard_rank, int shard_count, int layout, pm_pk **out) {
    if (!ctx || !a || !b || !c || !x_trapdoor || !z_trapdoor || !out) return PM_ERR_INVALID_ARG;
    return pk_entry(ctx, curve, [&](auto cv) {
        return pk_generate_impl<type_of<decltype(cv)>>(ctx, m0, mw, nr, a, b, c, x_trapdoor, z_trapdoor, shard_rank, shard_count, layout, out);
    });
}

extern "C" int pm_pk_generate(pm_ctx *ctx, int curve, uint64_t m0, uint64_t mw, uint64_t nr, const pm_csr *a,
                              const pm_csr *b, const pm_csr *c, const uint64_t *x_trapdoor, const uint64_t *z_trapdoor,
                              int shard_rank, int shard_count, pm_pk **out) {
    return pm_pk_generate_sharded(ctx, curve, m0, mw, nr, a, b, c, x_trapdoor, z_trapdoor, shard_rank, shard_count, PM_SHARD_PAIRS, out);
}

// ---- layout helpers for hosts and tests (polymath_amd/host/layout.hpp): pure index arithmetic, no GPU
extern "C" int pm_layout_indices(uint64_t n, int shard_count, int shard_rank, int coefficients, uint64_t *out /* n / shard_count */) {
    if (!out || shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count || !pmlayout::layout_ok(n, (uint32_t)shard_count)) return PM_ERR_INVALID_ARG;
    const pmlayout::Layout L = pmlayout::make_layout(n, (uint32_t)shard_count, (uint32_t)shard_rank);
    for (uint64_t p = 0; p < L.m; ++p) out[p] = coefficients ? pmlayout::coeff_global(L, p) : pmlayout::eval_global(L, p);
    return PM_OK;
}

extern "C" int pm_pk_msm_pieces(const pm_pk *pk, int which, uint64_t *cat_lo, uint64_t *count, size_t capacity, size_t *n_pieces) {
    if (!pk || which < 0 || which > 2 || !n_pieces) return PM_ERR_INVALID_ARG;
    *n_pieces = pk->pieces[which].size();
    for (size_t i = 0; i < pk->pieces[which].size() && i < capacity; ++i) {
        if (cat_lo) cat_lo[i] = pk->pieces[which][i].cat_lo;
        if (count) count[i] = pk->pieces[which][i].count;
    }
    return PM_OK;
}

extern "C" int pm_pk_info(const pm_pk *pk, uint64_t *n, uint64_t *m0, uint64_t *sigma, uint64_t *omega,
                          uint64_t base_lens[PM_NUM_BASE_VECS]) {
    if (!pk) return PM_ERR_INVALID_ARG;
    if (n) *n = pk->n;
    if (m0) *m0 = pk->m0;
    if (sigma) *sigma = pk->sigma;
    if (omega) memcpy(omega, pk->omega, 32);
    if (base_lens) for (int i = 0; i < PM_NUM_BASE_VECS; ++i) base_lens[i] = pk->base_len[i];
    return PM_OK;
}

// The witness solver's declared hints: PM_KEY_HINTS of pm_pk_load_bytes (below), stated as the call it is -- pm_pk_set_hints(ctx, pk,
// desc, n_words) -- because the set of entry points is pinned (host/solve_plan.hpp: decode_hints states the record format and every
// refusal).  The key is changed only when the whole declaration is accepted; a new generation number keeps a context from reusing a
// plan made under the old one (solve.hip: solve_plan).
static int pm_pk_set_hints(pm_ctx *ctx, pm_pk *pk, const uint64_t *desc, size_t n_words) {
    if (!ctx || !pk || (n_words && !desc)) return PM_ERR_INVALID_ARG;
    if (pk->shard_count != 1 || pk->layout != PM_SHARD_PAIRS) {
        ctx->err = "pm_pk_set_hints: hints on a sharded key are not supported";
        return PM_ERR_INVALID_ARG;
    }
    try {
        std::vector<pmsolve::Hint> hints;
        std::string why;
        const int st = pm::with_curve(pk->curve, [&](auto cv) {
            typedef typename pm::type_of<decltype(cv)>::FrP P;
            uint64_t modulus[4];
            for (int i = 0; i < 4; ++i) modulus[i] = (uint64_t)P::MOD[2 * i] | (uint64_t)P::MOD[2 * i + 1] << 32;
            why = pmsolve::decode_hints(desc, n_words, pk->m0 + pk->mw, modulus, hints);
            return (int)PM_OK;
        });
        if (st != PM_OK) return st;
        if (!why.empty()) {
            ctx->err = "pm_pk_set_hints: " + why;
            return PM_ERR_INVALID_ARG;
        }
        pk->hints.swap(hints);
        pk->hint_gen = pm::pk_serial_next();
    } catch (const std::bad_alloc &) {
        ctx->err = "pm_pk_set_hints: out of host memory";
        return PM_ERR_STATE;
    }
    return PM_OK;
}

extern "C" int pm_pk_msm_plan(const pm_pk *pk, int which, uint64_t *pairs, unsigned *windows, unsigned *window_bits, int *tables) {
    if (!pk || which < 0 || which > 2) return PM_ERR_INVALID_ARG;
    const uint64_t len = pk->res_cnt[which];
    unsigned nwin = 0, c = 0;
    if (pk->tables[which].planned()) {
        nwin = pk->tables[which].nwin;
        c = pk->tables[which].widest();
    } else {
        const uint64_t piece = len < pk->max_piece ? len : pk->max_piece;
        pm::msm_plan_query((size_t)piece, pk->curve == PM_BLS12_381 ? (unsigned)BlsFrP::BITS : (unsigned)BnFrP::BITS, &nwin, &c);
    }
    if (pairs) *pairs = len;
    if (windows) *windows = nwin;
    if (window_bits) *window_bits = c;
    if (tables) *tables = pk->tables[which].planned() && !pk->tables[which].wide ? 1 : 0;
    return PM_OK;
}

// Device element offset of [offset, offset + len) of base vector `which`; false if that range is not resident on this shard.
static bool pk_dev_range(const pm_pk *pk, int which, size_t offset, size_t len, uint64_t *dev_off) {
    const uint64_t lo = pk->seg_off[which] + offset, hi = lo + len;
    return pk->for_resident([&](uint64_t piece_lo, uint64_t count, uint64_t at) {
        if (lo < piece_lo || hi > piece_lo + count) return 0;
        *dev_off = at + (lo - piece_lo);
        return 1;
    }) != 0;
}

extern "C" int pm_pk_export_bases(pm_ctx *ctx, const pm_pk *pk, int which, size_t offset, size_t len, uint64_t *out_xy) {
    if (!ctx || !pk || !out_xy || which < 0 || which >= PM_NUM_BASE_VECS) return PM_ERR_INVALID_ARG;
    if (offset + len > pk->base_len[which]) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    size_t pt = pk->curve == PM_BLS12_381 ? sizeof(Affine<BlsCurve>) : sizeof(Affine<BnCurve>);
    uint64_t dev_off = 0;
    if (!pk_dev_range(pk, which, offset, len, &dev_off)) return PM_ERR_INVALID_ARG;  // not resident on this shard
    const void *src = (const uint8_t *)pk->d_bases + dev_off * pt;
    return with_curve(pk->curve, [&](auto cv) { return download_points<type_of<decltype(cv)>>(ctx, src, len, out_xy); });
}

// resident (internal-form) points -> standard form -> records of `form`, in chunks through the context's scratch
template <class C>
static int export_compressed_impl(pm_ctx *ctx, const Affine<C> *d_src, size_t len, int form, uint8_t *out) {
    const size_t NB = g1_record_bytes<C>(form), CH = wire_chunk(ctx), first = std::min(len, CH);
    PM_HIP(ctx, ctx->scratch.reserve(first * (sizeof(Affine<C>) + NB)));
    Affine<C> *d_pts = ctx->scratch.as<Affine<C>>();
    uint8_t *d_rec = (uint8_t *)(d_pts + first);   // sizeof(Affine<C>) = 96 / 64 bytes: 16-byte aligned
    for (size_t s = 0; s < len; s += CH) {
        const size_t cnt = std::min(CH, len - s);
        PM_HIP(ctx, hipMemcpyAsync(d_pts, d_src + s, cnt * sizeof(Affine<C>), hipMemcpyDeviceToDevice, ctx->stream));
        PM_TRY(bases_convert<C>(ctx, d_pts, cnt, false));
        PM_TRY(g1_encode_device<C>(ctx, d_pts, cnt, d_rec, form));
        PM_HIP(ctx, hipMemcpyAsync(out + s * NB, d_rec, cnt * NB, hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PM_OK;
}

extern "C" int pm_pk_export_bases_compressed(pm_ctx *ctx, const pm_pk *pk, int which, size_t offset, size_t len, uint8_t *out) {
    if (!ctx || !pk || !out || which < 0 || (which & ~(255 | PM_WIRE_UNCOMPRESSED))) return PM_ERR_INVALID_ARG;
    const int form = which & PM_WIRE_UNCOMPRESSED;      // which | PM_WIRE_UNCOMPRESSED: records of 96 / 64 bytes
    which &= 255;
    if (which >= PM_NUM_BASE_VECS) return PM_ERR_INVALID_ARG;
    if (offset + len > pk->base_len[which]) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    uint64_t dev_off = 0;
    if (!pk_dev_range(pk, which, offset, len, &dev_off)) return PM_ERR_INVALID_ARG;  // not resident on this shard
    if (!len) return PM_OK;
    return with_curve(pk->curve, [&](auto cv) {
        return export_compressed_impl<type_of<decltype(cv)>>(ctx, (const Affine<type_of<decltype(cv)>> *)pk->d_bases + dev_off, len, form, out);
    });
}

// -------------------------------------------------------------------------------- prove
// extern "C" entry points never let a C++ exception (bad_alloc in a host vector, system_error from a thread) unwind
// into the embedding host (a Rust shim or ctypes): it becomes a status with the message in pm_last_error.
template <class F>
static int guarded(pm_ctx *ctx, F body) {
    struct Turn {   // local serialised emulation (comm.hip): a phase runs holding the turn; no-op otherwise
        pm_comm *c;
        explicit Turn(pm_comm *cc) : c(cc) { if (c) c->phase_begin(); }
        ~Turn() { if (c) c->phase_end(); }
    } turn(ctx->comm);
    int st;
    try {
        st = body();
    } catch (const std::bad_alloc &) {
        ctx->err = "host allocation failed";
        st = PM_ERR_STATE;
    } catch (const std::exception &e) {
        ctx->err = e.what();
        st = PM_ERR_STATE;
    }
    // Fail-fast (include/polymath_hip.h, pm_comm contract): the prover's own verdicts are the same on every rank; any other
    // failure is this rank's alone, and its peers are about to wait for it in the next collective -- abort the communicator.
    const bool shared_verdict = st == PM_OK || st == PM_ERR_LEN_MISMATCH || st == PM_ERR_DOMAIN_TOO_LARGE || st == PM_ERR_REMAINDER_NONZERO ||
                                st == PM_ERR_DEGREE_BOUND || st == PM_ERR_INVALID_ARG;
    if (!shared_verdict && ctx->comm && !ctx->comm->failed) ctx->comm->abort(("a prover phase failed on this rank: " + ctx->err).c_str());
    return st;
}

extern "C" int pm_prove_phase1(pm_ctx *ctx, const pm_pk *pk, const uint64_t *x, const uint64_t *w, const uint64_t *r_a,
                               uint64_t *a_g1_xy, int *a_inf, uint64_t *c_g1_xy, int *c_inf) {
    if (!ctx || !pk || !x || !r_a || !a_g1_xy || !a_inf || !c_g1_xy || !c_inf || (pk->mw && !w)) return PM_ERR_INVALID_ARG;
    if (pk->device != ctx->device) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return guarded(ctx, [&] {
        return with_curve(pk->curve, [&](auto cv) {
            typedef type_of<decltype(cv)> C;
            return pk->layout == PM_SHARD_VECTOR ? prove_phase1_sharded<C>(ctx, pk, x, w, r_a, a_g1_xy, a_inf, c_g1_xy, c_inf, false)
                                                 : prove_phase1_impl<C>(ctx, pk, x, w, r_a, a_g1_xy, a_inf, c_g1_xy, c_inf, false);
        });
    });
}

extern "C" int pm_prove_phase1_device(pm_ctx *ctx, const pm_pk *pk, const uint64_t *d_x, const uint64_t *d_w, const uint64_t *r_a,
                                      uint64_t *a_g1_xy, int *a_inf, uint64_t *c_g1_xy, int *c_inf) {
    if (!ctx || !pk || !d_x || !r_a || !a_g1_xy || !a_inf || !c_g1_xy || !c_inf || (pk->mw && !d_w)) return PM_ERR_INVALID_ARG;
    if (pk->device != ctx->device) return PM_ERR_INVALID_ARG;
    PM_TRY(set_device(ctx));
    return guarded(ctx, [&] {
        return with_curve(pk->curve, [&](auto cv) {
            typedef type_of<decltype(cv)> C;
            return pk->layout == PM_SHARD_VECTOR ? prove_phase1_sharded<C>(ctx, pk, d_x, d_w, r_a, a_g1_xy, a_inf, c_g1_xy, c_inf, true)
                                                 : prove_phase1_impl<C>(ctx, pk, d_x, d_w, r_a, a_g1_xy, a_inf, c_g1_xy, c_inf, true);
        });
    });
}

extern "C" int pm_prove_phase2(pm_ctx *ctx, const uint64_t *x1, uint64_t *u_at_x1) {
    if (!ctx || !x1 || !u_at_x1) return PM_ERR_INVALID_ARG;
    if (!ctx->pk) return PM_ERR_STATE;
    PM_TRY(set_device(ctx));
    return guarded(ctx, [&] {
        return with_curve(ctx->pk->curve, [&](auto cv) {
            typedef type_of<decltype(cv)> C;
            return ctx->pk->layout == PM_SHARD_VECTOR ? prove_phase2_sharded<C>(ctx, x1, u_at_x1) : prove_phase2_impl<C>(ctx, x1, u_at_x1);
        });
    });
}

extern "C" int pm_prove_phase3(pm_ctx *ctx, const uint64_t *x1, const uint64_t *x2, const uint64_t *a_at_x1,
                               const uint64_t *c_at_x1, uint64_t *d_g1_xy, int *d_inf) {
    if (!ctx || !x1 || !x2 || !a_at_x1 || !c_at_x1 || !d_g1_xy || !d_inf) return PM_ERR_INVALID_ARG;
    if (!ctx->pk) return PM_ERR_STATE;
    PM_TRY(set_device(ctx));
    return guarded(ctx, [&] {
        return with_curve(ctx->pk->curve, [&](auto cv) {
            typedef type_of<decltype(cv)> C;
            return ctx->pk->layout == PM_SHARD_VECTOR ? prove_phase3_sharded<C>(ctx, x1, x2, a_at_x1, c_at_x1, d_g1_xy, d_inf)
                                                      : prove_phase3_impl<C>(ctx, x1, x2, a_at_x1, c_at_x1, d_g1_xy, d_inf);
        });
    });
}

extern "C" int pm_prove_tap(pm_ctx *ctx, int which, uint64_t *out, size_t max_elems, size_t *n_elems) {
    if (!ctx || !out || !n_elems) return PM_ERR_INVALID_ARG;
    if (which == 8) {   // the batch verifier's tap (verify_batch.hip): host memory, no proof in flight needed
        if (ctx->verify_tap.empty()) return PM_ERR_STATE;
        *n_elems = ctx->verify_tap.size() / 4;
        memcpy(out, ctx->verify_tap.data(), std::min(*n_elems, max_elems) * 32);
        return PM_OK;
    }
    if (which == 9) {   // the witness solver's small results (solve.hip): host memory
        if (ctx->sv.tap9.empty()) return PM_ERR_STATE;
        *n_elems = ctx->sv.tap9.size() / 4;
        memcpy(out, ctx->sv.tap9.data(), std::min(*n_elems, max_elems) * 32);
        return PM_OK;
    }
    if (which == 10) {  // ... and the completed rows of the last solving check call, in the context's device buffer
        if (!ctx->sv.tap10_rows) return PM_ERR_STATE;
        PM_TRY(set_device(ctx));
        *n_elems = ctx->sv.tap10_rows * ctx->sv.tap10_cols;
        const size_t k10 = std::min(*n_elems, max_elems);
        if (k10) PM_HIP(ctx, hipMemcpy(out, ctx->sv.xw.p, k10 * 32, hipMemcpyDeviceToHost));
        return PM_OK;
    }
    if (which == 11) {  // the device glue's challenges of the last pm_host_prove_batch with PM_PROVE_GLUE_DEVICE (prove_glue.hip): device buffer
        if (!ctx->gw.tap_rows) return PM_ERR_STATE;
        PM_TRY(set_device(ctx));
        *n_elems = ctx->gw.tap_rows * 4;
        const size_t k11 = std::min(*n_elems, max_elems);
        if (k11) PM_HIP(ctx, hipMemcpy(out, ctx->gw.tap.p, k11 * 32, hipMemcpyDeviceToHost));
        return PM_OK;
    }
    if (!ctx->pk || ctx->phase < 1) return PM_ERR_STATE;
    PM_TRY(set_device(ctx));
    const pm_pk *pk = ctx->pk;
    const pm::ProofShape shape = pm::proof_shape(pk);
    const uint64_t n = shape.n, Lz = shape.Lz;
    const void *src = nullptr;
    size_t cnt = 0;
    if (pk->layout == PM_SHARD_VECTOR) {
        // this rank's LOCAL vectors (coefficients in the blocked layout: pm_layout_indices); the evaluations are consumed
        // by the in-place transforms and are not available
        const uint64_t N = (uint64_t)pk->shard_count, q = (uint64_t)pk->shard_rank, m = n / N;
        const uint64_t zcnt = pmlayout::ztail_lo(Lz, (uint32_t)N, (uint32_t)q + 1) - pmlayout::ztail_lo(Lz, (uint32_t)N, (uint32_t)q);
        switch (which) {
            case 2: src = ctx->pw.u.p; cnt = m; break;
            case 3: src = ctx->pw.w.p; cnt = m; break;
            case 4: src = (const uint8_t *)ctx->pw.sc_c.p + zcnt * 32; cnt = m - (q == N - 1 ? 1 : 0); break;
            case 5: src = ctx->pw.wit_u.p; cnt = m; break;
            case 6: src = ctx->pw.sc_c.p; cnt = zcnt; break;
            case 7:
                if (ctx->phase < 3) return PM_ERR_STATE;
                src = ctx->pw.quotient.p; cnt = pk->res_cnt[2]; break;
            default: return PM_ERR_INVALID_ARG;
        }
        *n_elems = cnt;
        const size_t kk = std::min(cnt, max_elems);
        if (kk) PM_HIP(ctx, hipMemcpy(out, src, kk * 32, hipMemcpyDeviceToHost));
        return PM_OK;
    }
    switch (which) {
        case 0: src = ctx->pw.ue.p; cnt = n; break;
        case 1: src = ctx->pw.we.p; cnt = n; break;
        case 2: src = ctx->pw.u.p; cnt = n; break;
        case 3: src = ctx->pw.w.p; cnt = n; break;
        case 4: src = (const uint8_t *)ctx->pw.sc_c.p + Lz * 32; cnt = n - 1; break;
        case 5: src = ctx->pw.wit_u.p; cnt = n; break;
        case 6: src = ctx->pw.sc_c.p; cnt = Lz; break;
        case 7:
            if (ctx->phase < 3) return PM_ERR_STATE;
            src = ctx->pw.quotient.p; cnt = shape.len_d; break;
        default: return PM_ERR_INVALID_ARG;
    }
    *n_elems = cnt;
    size_t k = std::min(cnt, max_elems);
    PM_HIP(ctx, hipMemcpy(out, src, k * 32, hipMemcpyDeviceToHost));
    return PM_OK;
}
