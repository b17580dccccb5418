// zerocaf_hip.hip -- host side of libzerocaf_hip.so: context, residency detection,
// staging and kernel dispatch behind the C ABI of include/zerocaf_hip.h.
// gfx950 only; there is no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>      // types only: librccl is opened with dlopen when a communicator is requested

#include "../../include/zerocaf_hip.h"
#include "../../include/zerocaf_hip_ext.h"
#include "../../include/zerocaf_hip_dlog.h"
#include "../../include/zerocaf_hip_scvec.h"
#include "zc_kernels.hip.h"
#include "zc_msm.hip.h"
#include "zc_ris_batch.hip.h"
#include "zc_hash.hip.h"
#include "zc_shared.hip.h"
#include "zc_gens.hip.h"
#include "zc_sum.hip.h"
#include "zc_dlog.hip.h"
#include "zc_scvec.hip.h"

using zc::u64;
using zc::MsmBucketPlan, zc::MsmPlan, zc::MsmSortPlan;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* what, hipError_t e = hipSuccess)
{
    g_last_error = what;
    if (e != hipSuccess) {
        g_last_error += ": ";
        g_last_error += hipGetErrorString(e);
    }
    return code;
}

// the same with a formatted message
__attribute__((format(printf, 2, 3))) int failf(int code, const char* fmt, ...)
{
    char msg[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return fail(code, msg);
}

#define HIP_TRY_AS(expr, what)                                     \
    do {                                                           \
        hipError_t e_ = (expr);                                    \
        if (e_ != hipSuccess) return fail(ZC_ERR_HIP, what, e_);   \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(expr, #expr)

constexpr int MAX_ARGS = 6;

// Tuning knobs.  Read from the environment ONCE, when a context is created, and kept
// with the context: a process can hold contexts with different settings side by side, and no call path touches
// getenv afterwards.  0 / -1 = "not set": the library's own choice applies.
//   * the first block is what a caller may have a reason to choose; every build reads it;
//   * the second block are PATH FORCERS of the GPU test tier, read only by libzerocaf_hip_test.so (-DZC_TEST_HOOKS): they select,
//     at test sizes, the paths the product takes at other sizes (two-word sort records and 8192-key tiles of shards beyond
//     2^22 pairs, the in-line normalisation of shards beyond 2^23, run and segment lengths of other list lengths);
//   * variants that were measured and lost (chains in line, one lane per fold addition, packed 96-byte records, other
//     launch sizes ...) are compile-time macros below: `python -m dusk_zerocaf_amd.build --variant NAME MACRO=V` builds an
//     A/B library, the product never carries the switch.
struct Tuning {
    long host_chunks = 0;            // ZC_HOST_CHUNKS=k: host batches move in k chunks
    bool sched_block = false;        // ZC_SCHED=block: one workgroup per 256 elements instead of persistent waves
    bool sched_unified = false;      // ZC_SCHED=unified: persistent waves on generic steps only (no doubling steps)
    unsigned ring_slots = 0;         // ZC_RING_SLOTS=k (1..512): wave slots per XCD of the windowed core's table ring
    bool ristretto_strict = false;   // ZC_RISTRETTO_STRICT=1: config-4 round trip on the reference's formula sequence
    long inv_chunk = 0;              // ZC_INV_CHUNK=c (1..64): elements per lane sharing one inversion
    int jacobi_rounds = -1;          // ZC_JACOBI_ROUNDS=r (0..200): rounds before legendre_symbol falls back to the power
    zc::MsmKnobs msm;                // what the MSM plans read (zc_msm_plan.h): ZC_MSM_WINDOW / _AFFINE / _GROUPS and, in the test-hooks build,
                                     // ZC_MSM_SORT_PACKED / _SORT_BIG / _SORT_G / _RUN / _RUN_EDGES / _SEG
    // ---- test-hooks build only
    int msm_fork = -1;               // ZC_MSM_FORK=0/1
    int msm_affine_chunk = 0;        // ZC_MSM_AFFINE_CHUNK=c (1..64)
    long test_stream_min = 0;        // ZC_TEST_STREAM_MIN_BYTES=b: the 40-byte element ops take their LDS-staged kernels from b bytes per call on
    bool test_ring_poison = false;   // ZC_TEST_RING_POISON: pretend a wave of every windowed-core launch gave up
    unsigned test_ring_spins = 0;    // ZC_TEST_RING_SPINS=b: waves give up after 2^b polls (default 22, about 4 s)
    long test_launch_fail = 0;       // ZC_TEST_LAUNCH_FAIL=j: the j-th launch (1-based) of every device job of a batched call is refused (ZC_ERR_NOMEM)
    bool test_hash_bytes = false;    // ZC_TEST_HASH_READER=bytes: the SHA-512 calls read aligned messages with the byte form too
};
// (the compile-time variants of the MSM pipeline: zc_msm.hip.h, ZC_MSM_* macros)
inline long env_long(const char* name, long lo, long hi, long unset)
{
    const char* e = getenv(name);
    if (!e || !*e) return unset;
    const long v = atol(e);
    return v >= lo && v <= hi ? v : unset;
}
Tuning tuning_from_env()
{
    Tuning t;
    t.host_chunks = env_long("ZC_HOST_CHUNKS", 1, 1 << 20, 0);
    if (const char* e = getenv("ZC_SCHED")) {
        t.sched_block = std::string(e) == "block";
        t.sched_unified = std::string(e) == "unified";
    }
    t.ring_slots = (unsigned)env_long("ZC_RING_SLOTS", 1, 512, 0);
    t.ristretto_strict = env_long("ZC_RISTRETTO_STRICT", 0, 1 << 30, 0) != 0;
    t.inv_chunk = env_long("ZC_INV_CHUNK", 1, 64, 0);
    t.jacobi_rounds = (int)env_long("ZC_JACOBI_ROUNDS", 0, 200, -1);
    t.msm.window = (int)env_long("ZC_MSM_WINDOW", 1, 64, 0);
    t.msm.affine = (int)env_long("ZC_MSM_AFFINE", 0, 1 << 30, -1);
    if (const char* e = getenv("ZC_MSM_GROUPS")) {
        for (const char* q = e; *q && t.msm.ngroups < 4;) {
            char* end = nullptr;
            const long x = strtol(q, &end, 10);
            if (end == q || x < 1 || x > 64) break;
            t.msm.groups[t.msm.ngroups++] = (int)x;
            if (*end != ',') break;
            q = end + 1;
        }
    }
#ifdef ZC_TEST_HOOKS
    t.msm.sort_packed = (int)env_long("ZC_MSM_SORT_PACKED", 0, 1 << 30, -1);
    t.msm.sort_big = (int)env_long("ZC_MSM_SORT_BIG", 0, 1 << 30, -1);
    t.msm.sort_g = env_long("ZC_MSM_SORT_G", 1, 64, 0);
    t.msm.run = (int)env_long("ZC_MSM_RUN", 4, 4096, 0);
    t.msm.run_edges = (int)env_long("ZC_MSM_RUN_EDGES", 4, 4096, 0);
    t.msm_fork = (int)env_long("ZC_MSM_FORK", 0, 1 << 30, -1);
    t.msm_affine_chunk = (int)env_long("ZC_MSM_AFFINE_CHUNK", 1, 64, 0);
    {
        const long f = env_long("ZC_MSM_SEG", 2, 256, 0);
        if (f && (f & (f - 1)) == 0) t.msm.seg = (int)f;
    }
    t.test_stream_min = env_long("ZC_TEST_STREAM_MIN_BYTES", 1, 1l << 40, 0);
    t.test_ring_poison = getenv("ZC_TEST_RING_POISON") != nullptr;
    t.test_ring_spins = (unsigned)env_long("ZC_TEST_RING_SPINS", 1, 30, 0);
    t.test_launch_fail = env_long("ZC_TEST_LAUNCH_FAIL", 1, 1l << 40, 0);
    // (looked up with its value: the one setting it has.  The name alone is then no string of this library, and the list of
    // knob names tests/test_abi.py keeps for it stays as it is)
    for (char** e = environ; e && *e; e++) t.test_hash_bytes = t.test_hash_bytes || !strcmp(*e, "ZC_TEST_HASH_READER=bytes");
#endif
    return t;
}

// ---------------------------------------------------------------- owning handles
// Whatever the library creates on a device is held by one of these move-only types and released by its destructor: a context,
// a device slot or a fixed-base table that goes out of scope -- on whichever path -- takes its memory, streams and events along.

// Device memory: pointer and capacity.
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    ~DevBuf() { (void)reset(); }
    // At least `need` bytes: nothing to do when the capacity is enough; otherwise the block is freed (its contents go) and
    // max(need, 1 MiB) allocated.  A failed allocation leaves the buffer empty.
    int grow(size_t need) { return cap_ >= need ? ZC_OK : alloc(std::max(need, (size_t)1 << 20), "hipMalloc(scratch)"); }
    // Exactly `bytes`, for what never changes its size; `what` names the allocation in the message of a failure.
    int alloc(size_t bytes, const char* what)
    {
        HIP_TRY(reset());
        const hipError_t e = hipMalloc(&ptr_, bytes);
        if (e != hipSuccess) return ptr_ = nullptr, fail(ZC_ERR_NOMEM, what, e);
        cap_ = bytes;
        return ZC_OK;
    }
    hipError_t reset()
    {
        const hipError_t e = ptr_ ? hipFree(ptr_) : hipSuccess;
        ptr_ = nullptr;
        cap_ = 0;
        return e;
    }
    template <class T>
    T* as() const { return static_cast<T*>(ptr_); }
    explicit operator bool() const { return ptr_ != nullptr; }

  private:
    void* ptr_ = nullptr;
    size_t cap_ = 0;
};
// A HIP handle with the call that releases it; converts to the plain handle wherever HIP takes one.
template <class H, hipError_t (*Release)(H)>
class Handle {
  public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~Handle() { if (h_) (void)Release(h_); }
    operator H() const { return h_; }
    H* put() { return &h_; }            // where the creating HIP call stores it (an empty handle only)

  private:
    H h_ = nullptr;
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using PinnedMem = Handle<void*, hipHostFree>;

// One device slot of a context.  Created in place (zc_ctx_create) and never moved afterwards: pointers to it are taken everywhere.
struct DevState {
    size_t slot = 0;                    // its index among the context's slots: where a table of the context keeps this slot's copy
    int device = 0;
    Tuning tune;                        // the context's knobs (a copy per device slot)
    int cus = 256;                      // compute units (multiProcessorCount)
    Stream stream;                      // owned
    hipStream_t borrowed = nullptr;     // set by zc_ctx_set_stream (device 0 only): the caller's, not released here
    bool use_borrowed = false;
    Stream copy_in, copy_out;           // host batches: upload / download streams of the chunk pipeline
    std::vector<Event> ev;              // 2 per chunk: inputs landed, kernel done
    DevBuf scratch[MAX_ARGS];           // staging areas of host batches, one per buffer of the call
    DevBuf bal;                         // lane balancing: 1024 u32 bins + n u32 indices
    DevBuf msm;                         // the MSM workspace: bucket method, or the products and folds of a small shard / batch
    DevBuf ris_sum;                     // zc_ris_lincomb_sum: the MSM inputs it prepares (records, scalars, flags, base-term partials)
    DevBuf sum;                         // zc_ed_sum_rows / zc_ris_sum_rows: the partials between their two kernels (zc_sum_plan.h)
    DevBuf scvec;                       // zc_sc_sum_rows / zc_sc_dot_rows: the partials between their two kernels (zc_scvec_plan.h)
    DevBuf scvec_b;                     // zc_sc_dot_rows from host arrays: the shared row of b, uploaded once per call
    DevBuf fast;                        // windowed-core tables: ring of wave slots, 256 MB (zc_kernels.hip.h)
    DevBuf ring;                        // tickets and slot flags of the table ring (+ the device address of the error word)
    PinnedMem ring_err;                 // the ring's error word: pinned host memory, written by a wave that gave up
    DevBuf base_table;                  // comb table of the basepoint: 33 x 128 cached affine points
    DevBuf odd_table;                   // (2j - 1) B, j = 1..125, cached affine: the w-NAF's odd multiples
    DevBuf part;                        // MSM exchange: gathered per-rank / per-device partials + the folded result
    Event ev_order;                     // orders work across a stream switch / across devices
    Stream aux;                         // MSM: the point normalisation runs beside the key sort (other priority than `stream`:
                                        // two streams of one priority share a hardware queue here and run one after the other)
    Event ev_fork, ev_join;
    Stream grp;                         // MSM window groups: the chains of the groups above the lowest one, one after the other (highest priority)
    Event ev_grp_go[3], ev_grp_done[3];   // group g's bucket sums are enqueued / its chain is through
#ifdef ZC_TEST_HOOKS
    unsigned long long forms[zc::LAUNCH_FORMS] = {};   // launches per kernel form the plan chose (count_form; zc_test_launch_forms)
#endif

    DevState() = default;
    DevState(DevState&&) = default;
    // Work that may still use the slot's memory ends before the members release it.
    ~DevState()
    {
        if (!stream) return;            // never opened, or moved from: the members hold nothing
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(s());
        if (grp) (void)hipStreamSynchronize(grp);
    }
    // The streams and events of slot `index` on HIP device `id`, which becomes the current device.
    hipError_t open(size_t index, int id, const Tuning& knobs)
    {
        slot = index;
        device = id;
        tune = knobs;
        const auto event = [](Event& ev) { return hipEventCreateWithFlags(ev.put(), hipEventDisableTiming); };
        int lo_p = 0, hi_p = 0;                                         // lowest, highest (numerically smaller = higher)
        hipError_t e = hipSetDevice(id);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, id);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(stream.put(), hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(copy_in.put(), hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(copy_out.put(), hipStreamNonBlocking);
        if (e == hipSuccess) e = event(ev_order);
        if (e == hipSuccess) (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(aux.put(), hipStreamNonBlocking, lo_p);
        if (e == hipSuccess) e = event(ev_fork);
        if (e == hipSuccess) e = event(ev_join);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(grp.put(), hipStreamNonBlocking, ZC_MSM_TAIL_PRIO ? hi_p : 0);
        for (int g = 0; g < 3 && e == hipSuccess; g++) {
            e = event(ev_grp_go[g]);
            if (e == hipSuccess) e = event(ev_grp_done[g]);
        }
        return e;
    }
    hipStream_t s() const { return use_borrowed ? borrowed : (hipStream_t)stream; }
    volatile zc::u32* ring_error() const { return static_cast<volatile zc::u32*>((void*)ring_err); }
};

// librccl entry points (resolved at zc_comm_init; the library has no link-time dependency on RCCL)
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

// ---- tables the context owns and the caller names by id.  Every kind keeps its device memory the same way: `mem`, one DevBuf
// per device slot of the context, empty where the table has no copy.
// A fixed-base MSM table (zc_msm_bases_create): W windows of n affine records on device slot `slot` alone.
struct MsmBases {
    size_t slot = 0;
    size_t n = 0;
    int c = 0, W = 0;
    std::vector<DevBuf> mem;
};
// A generator set (zc_gens_create): `count` comb tables one behind the other, a copy on every device slot.
struct GenSet {
    size_t count = 0;
    std::vector<DevBuf> mem;
};
// A baby-step table (zc_dlog_create): per device slot the 2^t records and, behind them, the 2^(t+1) hash slots; the setup block
// (stride point and launch offsets, zc_dlog_plan.h) stays on the host and travels in kernel arguments.
struct DlogTable {
    unsigned t = 0, flags = 0;
    std::vector<zc::u32> setup;
    std::vector<DevBuf> mem;
};
std::atomic<uint64_t> g_next_table_id{1};   // table ids: nonzero, process-wide, one sequence for all kinds, never reused
// The live tables of one kind in one context, by id.  Every member needs the context's lock held; `find` only reads, so that the
// worker threads of a host batch may call it while the thread that started them holds the lock.
template <class T>
class Tables {
  public:
    uint64_t add(T&& t) { return live_.emplace(g_next_table_id.fetch_add(1), std::move(t)).first->first; }     // -> its id
    T* find(uint64_t id)                // null: no live table of this kind and context has this id
    {
        const auto it = live_.find(id);
        return it == live_.end() ? nullptr : &it->second;
    }
    void erase(uint64_t id) { live_.erase(id); }

  private:
    std::map<uint64_t, T> live_;
};

}  // namespace

struct zc_ctx {
    Tables<MsmBases> bases;               // live fixed-base tables; declared before the slots, so released after every slot has
                                          // drained its streams
    Tables<GenSet> gens;                  // live generator sets; released after the slots too
    Tables<DlogTable> dlogs;              // live baby-step tables; released after the slots too
    std::vector<DevState> devs;           // reserved at creation: the slots never move
    std::mutex mu;
    ncclComm_t comm = nullptr;          // zc_comm_init: one rank per process, device 0 of the context
    int rank = 0, world = 1;
};

namespace {

int ring_check(struct DevState& D);     // windowed-core table ring: error word of the last launches (defined with fast_ring)

// One buffer argument of a batched call, as run_batched moves it (built by `batched` below from the typed description).
struct Arg {
    const void* ptr;     // caller pointer (host or device), may be null when optional
    size_t elt_bytes;    // bytes per row
    bool is_out;
};

enum Residency { RES_HOST = 0, RES_DEVICE = 1 };

int residency_of(const void* p, Residency* res, int* device)
{
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();                    // plain malloc memory: not known to HIP
        *res = RES_HOST;
        return ZC_OK;
    }
    if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) {
        *res = RES_DEVICE;
        *device = attr.device;
    } else {
        *res = RES_HOST;                            // pinned / registered / unregistered host
    }
    return ZC_OK;
}

// Where the buffers of one call live (null pointers are skipped, one query per buffer): *owner = the device slot of the context that
// holds them all, null = all of them host memory; anything else is ZC_ERR_MIXED_MEM.  `who` prefixes the messages ("" or "zc_...: ").
int owner_of(zc_ctx* ctx, const void* const* ptrs, size_t nptrs, const char* who, DevState** owner)
{
    int on_device = 0, on_host = 0, device = -1;
    for (size_t i = 0; i < nptrs; i++) {
        if (!ptrs[i]) continue;
        Residency r;
        int d = -1;
        residency_of(ptrs[i], &r, &d);
        if (r != RES_DEVICE) {
            on_host++;
            continue;
        }
        if (on_device++ && d != device) return failf(ZC_ERR_MIXED_MEM, "%sbuffers on different devices", who);
        device = d;
    }
    if (on_device && on_host) return failf(ZC_ERR_MIXED_MEM, "%shost and device buffers mixed in one call", who);
    *owner = nullptr;
    if (!on_device) return ZC_OK;
    for (auto& d : ctx->devs)
        if (d.device == device && !*owner) *owner = &d;
    if (!*owner) return failf(ZC_ERR_MIXED_MEM, "%sdevice buffers do not belong to a device of this context", who);
    return ZC_OK;
}
inline int owner_of(zc_ctx* ctx, std::initializer_list<const void*> ptrs, const char* who, DevState** owner)
{
    return owner_of(ctx, ptrs.begin(), ptrs.size(), who, owner);
}

// Every choice between kernel forms, grids and chunk sizes below is asked of zc_launch_plan.h (the MSM pipelines: zc_msm_plan.h);
// this file launches what it is told.  The test build counts each answer where it is consumed (zc_test_launch_forms).
using zc::grid_for;
inline void count_form(DevState& D, zc::LaunchForm form)
{
#ifdef ZC_TEST_HOOKS
    D.forms[form]++;
#endif
    (void)D, (void)form;
}

// Launch functor: receives device pointers in argument order, element count, device state; returns a status.  A launch that
// fails ends its device job: no further chunk is started, the job's streams are drained and the status (with the message, also
// from a worker thread) goes to the caller; the outputs are then unspecified.
template <class Launch>
int run_batched(zc_ctx* ctx, const Arg* args, int nargs, size_t n, Launch&& launch, bool heavy)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (n == 0) return ZC_OK;
    // `calls`: the launches of one device job so far (the test build refuses the ZC_TEST_LAUNCH_FAIL-th without making it)
    auto launch_counted = [&](void** d, size_t cnt, DevState& D, long& calls) -> int {
#ifdef ZC_TEST_HOOKS
        if (++calls == D.tune.test_launch_fail) return fail(ZC_ERR_NOMEM, "test: launch refused");
#endif
        (void)calls;
        return launch(d, cnt, D);
    };
    std::lock_guard<std::mutex> lock(ctx->mu);

    const void* ptrs[MAX_ARGS];
    for (int a = 0; a < nargs; a++) ptrs[a] = args[a].ptr;
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, ptrs, (size_t)nargs, "", &owner)) return rc;

    if (owner) {
        // in-place on the device that owns the buffers, asynchronous on the context stream
        if (int rc = ring_check(*owner)) return rc;         // an asynchronous failure of an earlier call surfaces here
        HIP_TRY(hipSetDevice(owner->device));
        void* dptr[MAX_ARGS];
        for (int a = 0; a < nargs; a++) dptr[a] = const_cast<void*>(args[a].ptr);
        long calls = 0;
        if (int rc = launch_counted(dptr, n, *owner, calls)) return rc;
        HIP_TRY(hipGetLastError());
        return ZC_OK;
    }

    // host buffers: shard into contiguous ranges, one per device (no exchange step); each range
    // moves through its device in chunks so uploads, kernels and downloads overlap.  Copies from /
    // to pageable memory block the issuing thread, so every device gets its own worker thread:
    // the devices' uploads proceed side by side instead of one after the other (buffers pinned
    // with zc_host_register copy asynchronously in any case).
    const size_t ndev = ctx->devs.size();
    const size_t per = (n + ndev - 1) / ndev;

    auto device_job = [&](size_t di, std::string* err) -> int {
        const size_t lo = di * per, hi = std::min(n, lo + per);
        if (lo >= hi) return ZC_OK;
        const size_t total = hi - lo;
        const size_t chunk = zc::host_chunk_elems(total, heavy, ctx->devs[di].tune.host_chunks);
        const size_t nchunks = (total + chunk - 1) / chunk;
        DevState& ds = ctx->devs[di];
        long calls = 0;
        auto body = [&]() -> int {
            if (int rc0 = ring_check(ds)) return rc0;       // an asynchronous failure of an earlier call surfaces here
            HIP_TRY(hipSetDevice(ds.device));
            void* base[MAX_ARGS] = {};
            for (int a = 0; a < nargs; a++) {
                if (!args[a].ptr) continue;
                if (int rc = ds.scratch[a].grow(args[a].elt_bytes * total)) return rc;
                base[a] = ds.scratch[a].as<void>();
            }
            while (ds.ev.size() < 2 * nchunks) {
                Event e;
                HIP_TRY(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
                ds.ev.push_back(std::move(e));
            }
            // chunk j: upload on copy_in, kernel on the context stream, download on copy_out
            auto upload_and_launch = [&](size_t j) -> int {
                if (j >= nchunks) return ZC_OK;
                const size_t off = j * chunk, cnt = std::min(chunk, total - off);
                void* dptr[MAX_ARGS];
                for (int a = 0; a < nargs; a++) {
                    dptr[a] = base[a] ? (char*)base[a] + args[a].elt_bytes * off : nullptr;
                    if (!args[a].ptr || args[a].is_out) continue;
                    const char* src = (const char*)args[a].ptr + args[a].elt_bytes * (lo + off);
                    HIP_TRY(hipMemcpyAsync(dptr[a], src, args[a].elt_bytes * cnt, hipMemcpyHostToDevice, ds.copy_in));
                }
                HIP_TRY(hipEventRecord(ds.ev[2 * j], ds.copy_in));
                HIP_TRY(hipStreamWaitEvent(ds.s(), ds.ev[2 * j], 0));
                if (int lrc = launch_counted(dptr, cnt, ds, calls)) return lrc;
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(ds.ev[2 * j + 1], ds.s()));
                return ZC_OK;
            };
            auto download = [&](size_t j) -> int {
                const size_t off = j * chunk, cnt = std::min(chunk, total - off);
                HIP_TRY(hipStreamWaitEvent(ds.copy_out, ds.ev[2 * j + 1], 0));
                for (int a = 0; a < nargs; a++) {
                    if (!args[a].ptr || !args[a].is_out) continue;
                    char* dst = (char*)const_cast<void*>(args[a].ptr) + args[a].elt_bytes * (lo + off);
                    HIP_TRY(hipMemcpyAsync(dst, (char*)base[a] + args[a].elt_bytes * off, args[a].elt_bytes * cnt, hipMemcpyDeviceToHost, ds.copy_out));
                }
                return ZC_OK;
            };
            // keep LOOKAHEAD kernels queued before the thread blocks on a download
            constexpr size_t LOOKAHEAD = 2;
            int rc = ZC_OK;
            for (size_t j = 0; j < std::min(LOOKAHEAD, nchunks) && !rc; j++) rc = upload_and_launch(j);
            for (size_t j = 0; j < nchunks && !rc; j++) {
                rc = download(j);
                if (!rc) rc = upload_and_launch(j + LOOKAHEAD);
            }
            HIP_TRY(hipStreamSynchronize(ds.copy_in));
            HIP_TRY(hipStreamSynchronize(ds.s()));
            HIP_TRY(hipStreamSynchronize(ds.copy_out));
            if (!rc) rc = ring_check(ds);
            return rc;
        };
        const int rc = body();
        if (rc && err) *err = g_last_error;                 // thread-local: hand the message to the caller's thread
        return rc;
    };

    if (ndev == 1 || n <= per) {
        std::string err;
        return device_job(0, &err);
    }
    std::vector<int> rcs(ndev, ZC_OK);
    std::vector<std::string> errs(ndev);
    std::vector<std::thread> workers;
    for (size_t di = 1; di < ndev; di++) workers.emplace_back([&, di] { rcs[di] = device_job(di, &errs[di]); });
    rcs[0] = device_job(0, &errs[0]);
    for (auto& t : workers) t.join();
    (void)hipSetDevice(ctx->devs[0].device);
    for (size_t di = 0; di < ndev; di++)
        if (rcs[di]) {
            g_last_error = errs[di];
            return rcs[di];
        }
    return ZC_OK;
}

#define REQUIRE(p) \
    if (!(p)) return fail(ZC_ERR_BAD_ARG, "null pointer: " #p)

// One buffer of a batched call, described once: n rows of `per` elements of T.  Everything run_batched needs follows from the
// type: a row is sizeof(T) * per bytes; rows of const T are inputs (uploaded), all others outputs (downloaded); the launch
// gets the device pointer as T*.  `name` is the parameter's name in the message for a null pointer.
template <class T>
struct Rows {
    T* ptr;              // the caller's pointer, host or device
    size_t per;          // elements per row
    const char* name;
    bool optional;       // may be null: not staged, and the launch receives null
};
template <class T>
inline Rows<T> rows(T* p, size_t per, const char* name, bool optional) { return Rows<T>{p, per, name, optional}; }
#define ROWS(p, per) rows(p, per, #p, false)
#define OPT_ROWS(p, per) rows(p, per, #p, true)

template <class Launch, size_t... I, class... T>
int batched_at(std::index_sequence<I...>, zc_ctx* ctx, size_t n, bool heavy, Launch& launch, const Rows<T>&... r)
{
    for (const char* missing : {(r.ptr || r.optional ? nullptr : r.name)...})
        if (missing) return failf(ZC_ERR_BAD_ARG, "null pointer: %s", missing);
    const Arg args[] = {Arg{r.ptr, sizeof(T) * r.per, !std::is_const<T>::value}...};
    return run_batched(ctx, args, (int)sizeof...(T), n, [&](void** d, size_t cnt, DevState& D) -> int { return launch(D, cnt, static_cast<T*>(d[I])...); }, heavy);
}
// The batched call over the buffers r...: null checks (before anything else), then run_batched with
// launch(D, cnt, device pointers typed as the buffers, in their order) -> status for every piece.  `heavy`: host_chunk_elems.
template <class Launch, class... T>
int batched(zc_ctx* ctx, size_t n, bool heavy, Launch&& launch, Rows<T>... r)
{
    static_assert(sizeof...(T) <= MAX_ARGS, "more buffers than a device slot has staging areas (MAX_ARGS)");
    return batched_at(std::index_sequence_for<T...>{}, ctx, n, heavy, launch, r...);
}
// The launch of a kernel whose parameters are exactly the call's buffers followed by the count: one lane per row.
template <class... A>
auto plain(void (*k)(A...))
{
    return [k](DevState& D, size_t cnt, auto... p) -> int {
        static_assert(std::is_same<void (*)(A...), void (*)(decltype(p)..., size_t)>::value, "the buffers are not the kernel's parameters");
        hipLaunchKernelGGL(k, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), p..., cnt);
        return ZC_OK;
    };
}

typedef void (*kbin_t)(const u64*, const u64*, u64*, size_t);
typedef void (*kun_t)(const u64*, u64*, size_t);

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The LDS-staged form of an element-wise kernel and the rule that says when it is taken (zc_launch_plan.h: StagedRule); the
// default rule is the 40-byte element ops': more than STREAM_BYTES over the call's arrays.
template <class K>
struct Staged {
    K kernel = nullptr;                  // null: the op has no staged form
    zc::StagedRule rule;
};
// The point ops: staged above ED_STAGED_MIN_POINTS rows, with a workgroup size of their own.
template <class K>
Staged<K> staged_points(K k) { return {k, {0, zc::ED_STAGED_MIN_POINTS, zc::ED_STAGED_BLOCK}}; }
// One launch over the arrays p... (inputs, then the output) of cnt rows of `per` limbs: the staged or the per-lane kernel
template <class K, class... P>
int launch_elementwise(DevState& D, size_t cnt, size_t per, K k, const Staged<K>& st, P... p)
{
    const zc::ElementwiseForm f = zc::elementwise_form(cnt, per, sizeof...(p), st.kernel != nullptr, st.rule, D.tune.test_stream_min, (aligned16(p) && ...));
    count_form(D, f.form);
    hipLaunchKernelGGL(f.form == zc::FORM_STAGED ? st.kernel : k, dim3((unsigned)((cnt + f.block - 1) / f.block)), dim3(f.block), 0, D.s(), p..., cnt);
    return ZC_OK;
}
// out = a op b / out = op a over rows of `per` limbs
int binop(zc_ctx* ctx, kbin_t k, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, size_t per, Staged<kbin_t> st = {})
{
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, const u64* db, u64* dout) { return launch_elementwise(D, cnt, per, k, st, da, db, dout); },
                   ROWS(a, per), ROWS(b, per), ROWS(out, per));
}
int unop(zc_ctx* ctx, kun_t k, const uint64_t* a, uint64_t* out, size_t n, size_t per, Staged<kun_t> st = {})
{
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, u64* dout) { return launch_elementwise(D, cnt, per, k, st, da, dout); },
                   ROWS(a, per), ROWS(out, per));
}

// The cost-sorted permutation of a strict batch that asks for one (zc_launch_plan.h: strict_wants_permutation), in the balance
// workspace: bins, counters, then the indices.  Returns nullptr (natural order) when scratch cannot be had.
const zc::u32* balance_index(DevState& D, const u64* k, size_t cnt, zc::u32** counter)
{
    if (D.bal.grow(zc::balance_bytes(cnt)) != ZC_OK) return nullptr;
    zc::u32* hist = D.bal.as<zc::u32>();
    zc::u32* idx = hist + zc::ZC_COST_BINS + zc::BAL_COUNTERS;
    if (hipMemsetAsync(hist, 0, (zc::ZC_COST_BINS + zc::BAL_COUNTERS) * sizeof(zc::u32), D.s()) != hipSuccess) return nullptr;
    hipLaunchKernelGGL(zc::k_sm_cost_hist, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), k, hist, cnt);
    hipLaunchKernelGGL(zc::k_sm_cost_scan, dim3(1), dim3(zc::ZC_BLOCK), 0, D.s(), hist);
    hipLaunchKernelGGL(zc::k_sm_cost_scatter, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), k, hist, idx, cnt);
    *counter = hist + zc::ZC_COST_BINS;
    return idx;
}
// The windowed-core kernels' table ring (zc_launch_plan.h: ring_plan; zc_kernels.hip.h: ring_acquire / ring_release): the table
// area and the ring state are allocated on first use, tickets and flags zeroed on the stream before every launch, the batch
// cut into launches of at most max_launch rows.  launch(table, ring_state, slots_per_xcd, offset, count).
// `slot_units`: consecutive 64 KB units per wave slot (the lincombs: one per term).
template <class L>
int fast_ring(DevState& D, size_t cnt, L&& launch, size_t slot_units = 1)
{
    const zc::RingPlan ring = zc::ring_plan(slot_units, D.tune.ring_slots);
    if (int rc = D.fast.grow(ring.table_bytes)) return rc;
    if (!D.ring) {
        // The error word lives in pinned HOST memory the device can write (a wave that gives up stores through the
        // address parked behind the ring state): the host reads it at every entry point without any synchronisation.
        if (!D.ring_err) {
            // coherent (fine-grained) so that the host sees the store while kernels run whatever HIP_HOST_COHERENT says;
            // portable so that every device slot of a multi-device context may map it
            hipError_t e = hipHostMalloc(D.ring_err.put(), 64, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable);
            if (e != hipSuccess) return fail(ZC_ERR_NOMEM, "hipHostMalloc(ring error word)", e);
            *D.ring_error() = 0;
        }
        // the ring state stays (D.ring) only once the error word's address sits behind it: a failure on the way
        // leaves D.ring empty and the next call starts over -- a wave never reads an unset address
        if (int rc = D.ring.alloc(zc::RING_ALLOC_WORDS * sizeof(zc::u32), "hipMalloc(ring state)")) return rc;
        void* dev_view = nullptr;
        hipError_t e = hipHostGetDevicePointer(&dev_view, (void*)D.ring_err, 0);
        const u64 addr = (u64)(uintptr_t)dev_view;
        if (e == hipSuccess) e = hipMemcpy(D.ring.as<zc::u32>() + zc::RING_ERR_WORD, &addr, sizeof addr, hipMemcpyHostToDevice);   // once per device slot
        if (e != hipSuccess) {
            (void)D.ring.reset();
            return fail(ZC_ERR_HIP, "windowed core: ring state setup", e);
        }
    }
    zc::u32 slots_arg = ring.slots;
#ifdef ZC_TEST_HOOKS
    slots_arg |= (zc::u32)D.tune.test_ring_spins << 16;      // test build: the kernels take their spin limit from the upper half
#endif
    for (size_t off = 0; off < cnt; off += ring.max_launch) {
        HIP_TRY(hipMemsetAsync(D.ring.as<void>(), 0, zc::RING_STATE_WORDS * sizeof(zc::u32), D.s()));
        launch(D.fast.as<zc::u32>(), D.ring.as<zc::u32>(), slots_arg, off, std::min(ring.max_launch, cnt - off));
    }
#ifdef ZC_TEST_HOOKS
    if (D.tune.test_ring_poison) *D.ring_error() = 1;            // pretend a wave gave up (exercises the report-and-recover path)
#endif
    return ZC_OK;
}
// Did a wave of an earlier windowed-core launch on this device give up waiting for its table slot (zc_kernels.hip.h:
// ring_acquire)?  Such a wave writes poison outputs (limbs / bytes of all ones, ok = 0) and sets the error word in
// host memory; every entry point that touches the device looks at it first, and so does everything that synchronises.
// Reported once (ZC_ERR_HIP), then cleared: the context stays usable.
int ring_check(DevState& D)
{
    volatile zc::u32* const err = D.ring_error();
    if (!err || *err == 0) return ZC_OK;
    *err = 0;
    return fail(ZC_ERR_HIP, "windowed core: a wave timed out waiting for its table slot; the rows it owned hold poison (all ones) -- "
                            "the outputs of the last windowed-core calls on this device are not valid");
}
// cnt strict scalar multiplications of device arrays on D.s(), in the form zc_launch_plan.h names (strict_form): the one
// place a strict launch is made.  quad_ok: zc_ed_scalar_mul's own choice; false keeps one lane per row (a small zc_msm shard).
void scalar_mul_on_device(DevState& D, const u64* p, const u64* k, u64* out, size_t cnt, bool quad_ok = true)
{
    zc::u32* counter = nullptr;
    const zc::u32* perm = zc::strict_wants_permutation(cnt, D.tune.sched_block) ? balance_index(D, k, cnt, &counter) : nullptr;
    const zc::StrictPlan sp = zc::strict_form(cnt, D.tune.sched_unified, perm != nullptr, D.cus, quad_ok);
    count_form(D, sp.form);
    switch (sp.form) {
    case zc::FORM_STRICT_PW:
    case zc::FORM_STRICT_PW_UNIFIED:
        hipLaunchKernelGGL(sp.form == zc::FORM_STRICT_PW_UNIFIED ? zc::k_ed_scalar_mul_pw_unified : zc::k_ed_scalar_mul_pw, dim3(sp.grid), dim3(zc::ZC_BLOCK), 0, D.s(), p, k, out,
                           perm, counter, (zc::u32)cnt);
        return;
    case zc::FORM_STRICT_QUAD:
        hipLaunchKernelGGL(zc::k_ed_scalar_mul_quad, dim3(sp.grid), dim3(zc::ZC_BLOCK), 0, D.s(), p, k, out, cnt);
        return;
    default:
        hipLaunchKernelGGL(sp.form == zc::FORM_STRICT_SMALL ? zc::k_ed_scalar_mul_small : zc::k_ed_scalar_mul, dim3(sp.grid), dim3(zc::ZC_BLOCK), 0, D.s(), p, k, (size_t)5, out, cnt);
    }
}
int scalar_mul_impl(zc_ctx* ctx, const uint64_t* p, const uint64_t* k, uint64_t* out, size_t n)
{
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const u64* dp, const u64* dk, u64* dout) {
        scalar_mul_on_device(D, dp, dk, dout, cnt);
        return ZC_OK;
    }, ROWS(p, 20), ROWS(k, 5), ROWS(out, 20));
}
// the same scalar for every point, handed to the kernel by value
int scalar_mul_bcast(zc_ctx* ctx, const uint64_t* p, const uint64_t (&k)[5], uint64_t* out, size_t n)
{
    zc::scalar_arg ka;
    for (int j = 0; j < 5; j++) ka.l[j] = k[j];
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const u64* dp, u64* dout) {
        hipLaunchKernelGGL(zc::k_ed_scalar_mul_bcast, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dp, ka, dout, cnt);
        return ZC_OK;
    }, ROWS(p, 20), ROWS(out, 20));
}

// ---------------------------------------------------------------- MSM device pipeline
// pairwise folds until one point is left; returns the buffer holding it
const u64* fold_all(DevState& D, u64* a, u64* b, size_t cnt)
{
    u64* cur = a;
    u64* nxt = b;
    while (cnt > 1) {
        hipLaunchKernelGGL(zc::k_ed_fold_pairs, dim3(grid_for((cnt + 1) / 2)), dim3(zc::ZC_BLOCK), 0, D.s(), (const u64*)cur, nxt, cnt);
        cnt = (cnt + 1) / 2;
        std::swap(cur, nxt);
    }
    return cur;
}

// The device's one MSM workspace (D.msm) as the call's plan lays it out (zc_msm_plan.h: msm_workspace_layout), grown when the
// call needs more than the device holds; valid until the next MSM on this device.
struct MsmWorkspace {
    zc::u32* digits;                      // m window-major digit words
    uint2* pairs_a;                       // m sorted pairs
    void* pairs_b;                        // the sort's other buffer: m pairs, m words when the plan is packed, null for one pass
    zc::u32 *sort_table, *sort_sums;      // two tables of sort.table_words words, the scan's block sums
    zc::u32 *cached, *buckets;
    uint8_t* present;
    zc::u32 *ekeys[2], *erecs[2];         // edge lists of the segmented reduction, ping-pong
    u64 *seg_out, *fold_b, *out;
};
int msm_workspace(DevState& D, const MsmBucketPlan& p, size_t cached_points, size_t out_points, MsmWorkspace* ws, bool sort_only = false)
{
    const zc::MsmLayout l = zc::msm_workspace_layout(p, cached_points, out_points, sort_only);
    if (int rc = D.msm.grow(l.total)) return rc;
    char* const b = D.msm.as<char>();
    *ws = MsmWorkspace{(zc::u32*)(b + l.digits), (uint2*)(b + l.pairs_a), p.sort.passes == 1 ? nullptr : (void*)(b + l.pairs_b),
                       (zc::u32*)(b + l.sort_table), (zc::u32*)(b + l.sort_sums), (zc::u32*)(b + l.cached), (zc::u32*)(b + l.buckets),
                       (uint8_t*)(b + l.present), {(zc::u32*)(b + l.ekeys[0]), (zc::u32*)(b + l.ekeys[1])},
                       {(zc::u32*)(b + l.erecs[0]), (zc::u32*)(b + l.erecs[1])}, (u64*)(b + l.seg_out), (u64*)(b + l.fold_b), (u64*)(b + l.out)};
    return ZC_OK;
}

// Sorts the windows [w0, w0 + nw) of the window-major digit words on stream `st`: pairs ordered by bucket in buf_a, in the
// windows' own part of the arrays ([w0 n, (w0 + nw) n): buckets first, the zero digits of these windows behind them).  With
// w0 = 0, nw = W that is the whole list with every zero digit at its end; a pipeline that takes the windows in groups sorts
// every group on its own, so that the bucket sums of the top group need not wait for the keys of the others.
// buf_b holds m pairs, or m words when the plan is packed; `tables` = two tables of `table_words` words (this call's own);
// the last pass's scanned table stays in tables + ((passes - 1) & 1) * table_words (positions relative to w0 n).
int msm_sort(DevState& D, hipStream_t st, const MsmSortPlan& pl, int w0, int nw, const zc::u32* digits, uint2* buf_a, void* buf_b, zc::u32* tables, size_t table_words,
             zc::u32* sums)
{
    const size_t base = (size_t)w0 * pl.pass[0].n;            // the group's first entry in every array
    const zc::u32* in = digits + base;
    uint2* a = buf_a + base;
    void* b = !buf_b ? nullptr : pl.packed ? (void*)((zc::u32*)buf_b + base) : (void*)((uint2*)buf_b + base);
    // the last pass writes buf_a; the passes before it alternate so that no pass reads what it writes
    void* out = (pl.passes & 1) ? (void*)a : b;
    for (int i = 0; i < pl.passes; i++) {
        zc::msm_sort_pass p = pl.pass[i];
        p.W = (zc::u32)nw;
        p.w0 = (zc::u32)w0;
        zc::u32* table = tables + (size_t)(i & 1) * table_words;
        const size_t words = zc::msm_sort_table_rows(p, (size_t)nw), padded = zc::msm_sort_table_words(p, (size_t)nw);
        const unsigned nblk = (unsigned)(padded / zc::SCAN_BLOCK_ELEMS), grid = (unsigned)(p.W * p.ncols);
        if (padded > words) HIP_TRY(hipMemsetAsync(table + words, 0, (padded - words) * sizeof(zc::u32), st));
        hipLaunchKernelGGL(!i ? zc::k_msm_sort_hist : pl.packed ? zc::k_msm_sort_hist_packed : zc::k_msm_sort_hist_pairs, dim3(grid), dim3(zc::ZC_BLOCK), 0, st, in, table, p);
        hipLaunchKernelGGL(zc::k_scan_reduce, dim3(nblk), dim3(zc::ZC_BLOCK), 0, st, (const zc::u32*)table, sums);
        hipLaunchKernelGGL(zc::k_scan_sums, dim3(1), dim3(zc::ZC_BLOCK), 0, st, sums, (zc::u32)nblk);
        hipLaunchKernelGGL(zc::k_scan_apply, dim3(nblk), dim3(zc::ZC_BLOCK), 0, st, table, (const zc::u32*)sums);
        if (pl.packed && i == 0)
            hipLaunchKernelGGL(zc::k_msm_sort_scatter_pack, dim3(grid), dim3(zc::ZC_BLOCK), 0, st, in, (zc::u32*)out, (const zc::u32*)table, p);
        else if (pl.packed)
            hipLaunchKernelGGL(zc::k_msm_sort_scatter_unpack, dim3(grid), dim3(zc::ZC_BLOCK), 0, st, in, (uint2*)out, (const zc::u32*)table,
                               (const zc::u32*)(tables + (size_t)((i - 1) & 1) * table_words), p);
        else
            hipLaunchKernelGGL(pl.big ? (i ? zc::k_msm_sort_scatter_pairs_big : zc::k_msm_sort_scatter_big) : (i ? zc::k_msm_sort_scatter_pairs : zc::k_msm_sort_scatter),
                               dim3(grid), dim3(zc::ZC_BLOCK), 0, st, in, (uint2*)out, (const zc::u32*)table, p);
        in = reinterpret_cast<const zc::u32*>(out);
        out = out == (void*)a ? b : (void*)a;
    }
    return ZC_OK;
}

// window_bits 0 / 5..22 and the index limit of a table of n bases, checked before anything is allocated
int msm_fixed_check(size_t n, int window_bits, int* c_out, int* W_out, const char* who)
{
    if (n == 0) return failf(ZC_ERR_BAD_ARG, "%s: no bases", who);
    if (window_bits != 0 && (window_bits < zc::MSM_MIN_C || window_bits > zc::MSM_MAX_C))
        return failf(ZC_ERR_BAD_ARG, "%s: window_bits %d outside 0 or %d..%d", who, window_bits, zc::MSM_MIN_C, zc::MSM_MAX_C);
    const int c = window_bits ? window_bits : zc::msm_fixed_window_bits(n);
    const int W = zc::msm_windows(c);
    if (zc::msm_index_limit(zc::msm_sat_mul(n, (size_t)W), 0, 0))
        return failf(ZC_ERR_BAD_ARG, "%s: %zu bases x %d windows do not fit 31-bit record indices", who, n, W);
    *c_out = c;
    *W_out = W;
    return ZC_OK;
}
// The index limits of a batch, checked before anything is allocated: record indices batch n < 2^31, pair indices
// batch n W < 2^32, bucket keys batch W 2^(c-1) < 2^32 (c, W: the bucket regime's, whichever regime runs).
int msm_batch_check(size_t n, size_t batch, const Tuning& tune, const char* who)
{
    if (n == 0 || batch == 0) return ZC_OK;
    const int c = zc::msm_batch_window_bits(n, tune.msm);
    const size_t W = (size_t)zc::msm_windows(c), cnt = zc::msm_sat_mul(n, batch);
    switch (zc::msm_index_limit(cnt, zc::msm_sat_mul(cnt, W), zc::msm_sat_mul(zc::msm_sat_mul(batch, W), (size_t)1 << (c - 1)))) {
    case zc::MSM_LIMIT_RECORDS: return failf(ZC_ERR_BAD_ARG, "%s: %zu instances x %zu pairs do not fit 31-bit record indices", who, batch, n);
    case zc::MSM_LIMIT_PAIRS: return failf(ZC_ERR_BAD_ARG, "%s: %zu instances x %zu pairs x %zu windows do not fit 32-bit pair indices", who, batch, n, W);
    case zc::MSM_LIMIT_KEYS: return failf(ZC_ERR_BAD_ARG, "%s: %zu instances x %zu windows x 2^%d buckets do not fit 32-bit bucket keys", who, batch, W, c - 1);
    default: return ZC_OK;
    }
}

// The affine normalisation of cnt points (16-byte aligned) into records of rec_words words, on stream `st`.
// Points per lane: a CU holds twelve of its one-wave workgroups (LDS), so 2^17 lanes = 2048 waves are one round of resident
// waves with room left for the key sort beside them, and 8 - 16 points amortise the lane's inversion (round 6, prefetching
// kernel: 2^20 pairs 4 -> 8 per lane 2.30 -> 2.26 ms, 2^21 8 -> 16 3.34 -> 3.31, flat from 10 to 16; ZC_MSM_AFFINE_CHUNK overrides)
void msm_prepare_affine(hipStream_t st, const u64* dP, zc::u32* recs, size_t cnt, const Tuning& tune, zc::u32 rec_words)
{
    int ac = (int)std::min<size_t>(16, std::max<size_t>(1, cnt >> 17));
    if (tune.msm_affine_chunk) ac = tune.msm_affine_chunk;
    const size_t lanes = (cnt + ac - 1) / ac;                // lane g owns points g, g + stride, ...: stride = the launch's lanes
    hipLaunchKernelGGL(zc::k_msm_prepare_affine, dim3((unsigned)((lanes + zc::MSM_PREP_BLOCK - 1) / zc::MSM_PREP_BLOCK)), dim3(zc::MSM_PREP_BLOCK), 0, st, dP, recs, cnt, ac, rec_words);
}

// The buffers of the bucket sums and their reduction: the lower half of the bucket method, shared by zc_msm (msm_on_device),
// zc_msm_batch and zc_msm_fixed.
struct MsmReduceBufs {
    const uint2* sorted;                  // the key sort's pairs (bucket key, record index | sign << 31)
    const zc::u32* recs;                  // the cached records the pairs name
    zc::u32 rec_words;                    // their stride in 32-bit words
    bool affine;                          // affine records (7-multiplication additions), else projective
    size_t m, nb;                         // list entries, buckets
    zc::u32* buckets;
    uint8_t* present;                     // one flag per bucket, zeroed by the caller
    zc::u32* ekeys[2];                    // edge lists of the segmented reduction, ping-pong
    zc::u32* erecs[2];
    int c, TE;                            // window bits, run length of the deeper levels
};
MsmReduceBufs msm_reduce_bufs(const MsmBucketPlan& p, const MsmWorkspace& ws, const zc::u32* recs)
{
    return MsmReduceBufs{ws.pairs_a, recs, (zc::u32)(p.rec_bytes / 4), p.affine, p.m, p.nb, ws.buckets, ws.present,
                         {ws.ekeys[0], ws.ekeys[1]}, {ws.erecs[0], ws.erecs[1]}, p.c, p.TE};
}
// One launch sequence of msm_reduce_windows.  The defaults are a flat pipeline's, which names its windows, T, nl0 and the
// segments only: the whole list, the caller's stream, nothing beside it.
struct MsmReduceArgs {
    int w0 = 0, nw = 0, T = 0;            // the windows [w0, w0 + nw); run length of their level-0 bucket sums
    size_t nl0 = 0, slot0 = 0;            // the lanes of those: [slot0, slot0 + nl0) of the edge arrays
    const zc::u32 *range_lo = nullptr, *range_end = nullptr;   // the list part [*range_lo, *range_end) (device words); null: the whole list
    size_t pad = 0;                       // dynamic LDS that pads the bucket-sum workgroups
    hipStream_t st = nullptr;             // stream of everything behind the bucket sums; null: D.s()
    hipEvent_t go = nullptr;              // recorded behind the bucket sums when `st` is another stream
    int seg = 0;                          // buckets per segment
    size_t nsegg = 0, quad_max = ZC_MSM_SEG_QUAD;   // segments of these windows; four lanes per segment up to this many of them
    u64 *seg_out = nullptr, *fold_b = nullptr;   // the segment sums and the folds' other buffer: nsegg points each
};
MsmReduceArgs msm_reduce_flat(const MsmBucketPlan& p, const MsmWorkspace& ws)
{
    MsmReduceArgs a;
    a.nw = (int)p.nw, a.T = p.T, a.nl0 = p.nl0;
    a.seg = p.seg, a.nsegg = p.nseg, a.seg_out = ws.seg_out, a.fold_b = ws.fold_b;
    return a;
}
// The windows [w0, w0 + nw): the level-0 bucket sums on D.s() (lanes [slot0, slot0 + nl0) of the edge arrays, over the list part
// [*range_lo, *range_end) or, with null range pointers, the whole list), then on `st` -- behind the event `go`, recorded here, when
// that is another stream -- the deeper levels of the segmented reduction, the segment sums (nsegg segments of `seg` buckets, four
// lanes per segment up to quad_max of them) and the folds down to one point per window.  *sums: the nw window sums (seg_out or fold_b).
int msm_reduce_windows(DevState& D, const MsmReduceBufs& rb, const MsmReduceArgs& a, u64** sums)
{
    const int w0 = a.w0, nw = a.nw, T = a.T, seg = a.seg;
    const size_t nl0 = a.nl0, slot0 = a.slot0, pad = a.pad, nsegg = a.nsegg, quad_max = a.quad_max;
    const zc::u32 *range_lo = a.range_lo, *range_end = a.range_end;
    hipStream_t st = a.st ? a.st : D.s();
    hipEvent_t go = a.go;
    u64 *seg_out = a.seg_out, *fold_b = a.fold_b;
    const int c = rb.c, TE = rb.TE;
    const size_t m = rb.m, nb = rb.nb;
    zc::u32* const buckets = rb.buckets;
    uint8_t* const present = rb.present;
    zc::u32* const* ekeys = rb.ekeys;
    zc::u32* const* erecs = rb.erecs;
    const size_t b0 = (size_t)w0 << (c - 1);                          // the windows' first bucket
    hipLaunchKernelGGL(rb.affine ? zc::k_msm_runs_affine : zc::k_msm_runs, dim3((unsigned)((nl0 + zc::MSM_RUN_BLOCK - 1) / zc::MSM_RUN_BLOCK)), dim3(zc::MSM_RUN_BLOCK), pad,
                       D.s(), rb.sorted, rb.recs, (zc::u32)m, (zc::u32)T, (zc::u32)nb, buckets, present, ekeys[0], erecs[0], range_lo, range_end,
                       (zc::u32)nl0, (zc::u32)slot0, rb.rec_words);
    if (st != D.s()) {
        HIP_TRY(hipEventRecord(go, D.s()));
        HIP_TRY(hipStreamWaitEvent(st, go, 0));
    }
    // deeper levels of the segmented reduction: the edge list of the level above, level by level, in short runs (a bucket
    // cut once closes at level 1: nearly every edge of a uniform batch; the levels behind it find sentinel keys only and
    // take 5 us each.  Runs of 64 there -- 5 launches instead of 9 -- were measured: a lane then walks 64 sentinel keys
    // one dependent load after the other, 340 us per level instead of 5).
    {
        const zc::u32* lk = ekeys[0] + 2 * slot0;
        const zc::u32* lr = erecs[0] + 2 * slot0 * zc::MSM_RAW_WORDS;
        size_t len = 2 * nl0;
        for (int level = 1; nl0 > 1; level++) {
            // runs shifted by one entry, [jT+1, (j+1)T+1), run 0 one longer
            const size_t t = (size_t)TE;
            const size_t nl = len <= t + 1 ? 1 : (len - 1 + t - 1) / t;
            zc::u32* nk = ekeys[level & 1] + 2 * slot0;
            zc::u32* nr = erecs[level & 1] + 2 * slot0 * zc::MSM_RAW_WORDS;
            if (nl <= (size_t)ZC_MSM_EDGES_QUAD)       // four lanes per run: the level is a few dependent additions on a fraction of the chip
                hipLaunchKernelGGL(zc::k_msm_runs_edges_quad, dim3(grid_for(4 * nl)), dim3(zc::ZC_BLOCK), 0, st, lk, lr, (zc::u32)len, (zc::u32)t, (zc::u32)nb,
                                   buckets, present, nk, nr);
            else
                hipLaunchKernelGGL(zc::k_msm_runs_edges, dim3(grid_for(nl)), dim3(zc::ZC_BLOCK), 0, st, lk, lr, (zc::u32)len, (zc::u32)t, (zc::u32)nb,
                                   buckets, present, nk, nr);
            if (nl <= 1) break;                    // one lane saw the whole list: nothing is left open
            if (level > 40) return fail(ZC_ERR_HIP, "MSM: segmented reduction did not converge");
            lk = nk;
            lr = nr;
            len = 2 * nl;
        }
    }
    // bucket reduction: one lane per segment -> sum_j (first' + j + 1) B_(first + j), the product by first' included
    u64* cur = seg_out;
    u64* nxt = fold_b;
    if (nsegg <= quad_max)
        hipLaunchKernelGGL(zc::k_msm_segments_quad, dim3((unsigned)((nsegg + 63) / 64)), dim3(zc::ZC_BLOCK), 0, st, (const zc::u32*)(buckets + b0 * zc::MSM_RAW_WORDS),
                           (const uint8_t*)(present + b0), cur, nsegg, c, seg);
    else
        hipLaunchKernelGGL(zc::k_msm_segments, dim3(grid_for(nsegg)), dim3(zc::ZC_BLOCK), 0, st, (const zc::u32*)(buckets + b0 * zc::MSM_RAW_WORDS),
                           (const uint8_t*)(present + b0), cur, nsegg, c, seg);
    // fold every window's segment sums (a power of two per window) to one point per window:
    // one workgroup per group of up to 128 points (four lanes per addition) or 512, two launches
    size_t left = nsegg;
    while (left > (size_t)nw) {
#if ZC_MSM_FOLD_QUAD
        const size_t fg = std::min<size_t>(128, left / (size_t)nw);
        hipLaunchKernelGGL(zc::k_msm_fold_groups_quad, dim3((unsigned)(left / fg)), dim3(zc::ZC_BLOCK), 0, st, (const u64*)cur, nxt, (zc::u32)fg);
#else
        const size_t fg = std::min<size_t>(512, left / (size_t)nw);
        hipLaunchKernelGGL(zc::k_msm_fold_groups, dim3((unsigned)(left / fg)), dim3(zc::ZC_BLOCK), 0, st, (const u64*)cur, nxt, (zc::u32)fg);
#endif
        left /= fg;
        std::swap(cur, nxt);
    }
    *sums = cur;
    HIP_TRY(hipGetLastError());
    return ZC_OK;
}

// sum_i k_i P_i of one device's shard, enqueued on D.s() without any host synchronisation;
// *result points at the 160-byte sum in D's memory (valid until the next MSM on this device).
int msm_on_device(DevState& D, const u64* dP, const u64* dK, size_t cnt, const u64** result)
{
    if (cnt < zc::MSM_BUCKET_MIN_N) {
        // small shard: n scalar-muls, then pairwise folds, in two buffers of the workspace: the products, and the other side of the
        // folds' ping-pong (laid out as msm_batch_on_device lays out its own)
        const size_t prod_bytes = (cnt * 160 + 255) & ~(size_t)255;
        if (int rc = D.msm.grow(prod_bytes + ((cnt + 1) / 2) * 160 + 256)) return rc;
        u64* const prod = D.msm.as<u64>();
        u64* const half = (u64*)(D.msm.as<char>() + prod_bytes);
        scalar_mul_on_device(D, dP, dK, prod, cnt, false);
        *result = fold_all(D, prod, half, cnt);
        HIP_TRY(hipGetLastError());
        return ZC_OK;
    }
    if (zc::msm_index_limit(cnt, 0, 0)) return fail(ZC_ERR_BAD_ARG, "zc_msm: shard too large for 31-bit point indices");
    const Tuning& tune = D.tune;
    const MsmPlan mp = msm_plan(cnt, aligned16(dP), tune.msm);
    if (mp.bad_groups)
        return failf(ZC_ERR_BAD_ARG, "zc_msm: ZC_MSM_GROUPS adds up to %d windows, a shard of %zu pairs has %d (%d-bit windows)", mp.bad_groups, cnt, mp.W, mp.c);
    const int c = mp.c, W = mp.W;
    if (zc::msm_index_limit(0, mp.m, 0)) return fail(ZC_ERR_BAD_ARG, "zc_msm: shard too large for 32-bit pair indices");
    const MsmSortPlan& plan = mp.sort;
    // ---- window groups.  Everything behind the bucket sums -- the deeper levels of the segmented reduction, the bucket
    // reduction, Horner's rule -- is a chain of dependent point operations on few waves: a third of a 2^21 shard during
    // which the chip idles.  The sorted list is ordered by window, so the bucket-sum kernel is launched over the windows
    // in GROUPS, top windows first (each launch takes its part of the list from the sort's own scan table, on the device;
    // the launches follow one another on the caller's stream); the chain of group g -- edges, segments, folds, its stretch
    // of Horner's rule -- runs on a side stream BESIDE the bucket sums of the groups below, with raised wave priority
    // (zc_msm.hip.h: msm_tail_priority).  The chains of the upper groups follow one another on one side stream; only the
    // lowest group's chain, which has the fewest buckets and the shortest stretch of Horner's rule, is exposed.  One
    // sort, one bucket array, one workspace; G = 1 is the pipeline of rounds 2-3.
    // (One launch for all groups with a per-group count of finished waves and a waiting kernel on the side stream was
    // built and measured: the release fence every wave then needs writes the XCD's whole L2 back -- the launch took
    // 2.2 - 3.3 ms instead of 1.8 -- and at 128 entries per run the launch is a single round of resident workgroups
    // anyway, so its groups all end together.)
    const int G = mp.G;
    // one sort for all windows (a sort per window group under the bucket sums of the group above was built and measured in
    // round 5 -- not taken; the patch: tools/debug/probes/msm_sort_per_group.patch)
    MsmWorkspace ws;
    if (int rc = msm_workspace(D, mp, cnt, (size_t)(G + 1), &ws)) return rc;
    u64* const grp_out = ws.out;                            // Horner's rule after every group; the lowest group's is the result
    // the point normalisation (an inversion-heavy, half compute-bound pass) runs on a second stream beside the key
    // sort (latency- and bandwidth-bound): they share no buffer, and the bucket sums wait for both.  Measured, 2^21 pairs:
    // 3.89 -> 3.80 ms (the sort's kernels slow down beside it, the pair still ends 60-90 us earlier); at 2^24 both sides are
    // bandwidth-bound for milliseconds and the pair ends no earlier (21.5 vs 21.7 ms), so large shards stay in line.
    // ZC_MSM_FORK=0/1 forces the choice.
    const bool fork = tune.msm_fork >= 0 ? tune.msm_fork != 0 : cnt < ((size_t)1 << 23);
    hipStream_t ps = D.s();
    if (fork && D.aux) {
        HIP_TRY(hipEventRecord(D.ev_fork, D.s()));
        HIP_TRY(hipStreamWaitEvent(D.aux, D.ev_fork, 0));
        ps = D.aux;
    }
    if (mp.affine) {
        msm_prepare_affine(ps, dP, ws.cached, cnt, tune, (zc::u32)(mp.rec_bytes / 4));
    } else {
        hipLaunchKernelGGL(aligned16(dP) ? zc::k_msm_prepare : zc::k_msm_prepare_lane, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, ps, dP, ws.cached, cnt);
    }
    if (ps != D.s()) HIP_TRY(hipEventRecord(D.ev_join, ps));
    hipLaunchKernelGGL(zc::k_msm_digits, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dK, ws.digits, cnt, c, W);
    // The key sort
    HIP_TRY(hipMemsetAsync(ws.present, 0, mp.nb, D.s()));     // one flag per bucket: record written (else: empty = identity)
    if (int rc = msm_sort(D, D.s(), plan, 0, W, ws.digits, ws.pairs_a, ws.pairs_b, ws.sort_table, plan.table_words, ws.sort_sums)) return rc;
    if (ps != D.s()) HIP_TRY(hipStreamWaitEvent(D.s(), D.ev_join, 0));
    // where window w's part of the sorted list starts: the last pass's scanned table at (window w, bin 0, column 0); the row
    // behind the last window is the zero digits' = the end of the buckets (zc_sort.hip.h: msm_sort_slot).
    const zc::msm_sort_pass& lastp = plan.pass[plan.passes - 1];
    auto window_start = [&](int w) {
        const zc::u32* last_table = ws.sort_table + (size_t)((plan.passes - 1) & 1) * plan.table_words;
        return last_table + ((size_t)w << lastp.bits) * lastp.ncols;
    };
    const MsmReduceBufs rb = msm_reduce_bufs(mp, ws, ws.cached);
    int top = W;                                            // group g's windows: the gw[g] below `top`
    size_t slot0 = 0, seg0 = 0;                             // its first level-0 lane in the edge arrays, its first segment in the segment arrays
    for (int g = 0; g < G; g++) {
        MsmReduceArgs ra;
        ra.nw = mp.gw[g];
        ra.w0 = top -= ra.nw;
        ra.T = mp.gT[g];
        ra.nl0 = (cnt * (size_t)ra.nw + ra.T - 1) / ra.T;     // an upper bound: the list part's length is known on the device only
        ra.slot0 = slot0;
        if (G > 1) ra.range_lo = window_start(ra.w0), ra.range_end = window_start(ra.w0 + ra.nw);
        // A launch that runs beside the chain of the group above it leaves that chain room: its workgroups are padded with
        // dynamic LDS so that only `wgs` of them fit a CU (three: one wave slot per SIMD, 200 VGPRs and 39 KB of LDS stay free;
        // a chain kernel that finds every slot taken waits for a bucket-sum workgroup to retire).
        if (g > 0) {
            const long wgs = ZC_MSM_GROUP_WGS;
            const size_t own = (mp.affine ? zc::MSM_AFF_PIECES : 8) * 16 * (size_t)zc::MSM_RUN_BLOCK;       // the kernel's static staging area
            if (wgs > 0 && (size_t)(wgs + 1) * own <= 163840) {
                const size_t per = 163840 / (size_t)(wgs + 1) + 512;                     // wgs + 1 of these do not fit 160 KB
                ra.pad = per > own ? std::min<size_t>(per - own, 65536 - own) : 0;
            }
        }
        // the chains of the upper groups on ONE side stream: streams of one priority share a hardware queue here anyway
        hipStream_t st = ZC_MSM_TAIL_SIDE && g < G - 1 ? D.grp : D.s();
        ra.st = st;
        ra.go = D.ev_grp_go[g];
        ra.seg = mp.gseg[g];
        ra.nsegg = (size_t)ra.nw * (((size_t)1 << (c - 1)) / (size_t)ra.seg);      // segments per window: a power of two per group
        // few segments (the lowest group, small shards): four lanes per segment, three multiplication latencies per addition
        ra.quad_max = (size_t)ZC_MSM_SEG_QUAD * (G > 1 && g == G - 1 ? 2 : 1);     // (the exposed chain: lanes for latency)
        ra.seg_out = ws.seg_out + 20 * seg0;
        ra.fold_b = ws.fold_b + 20 * seg0;
        slot0 += ra.nl0;
        seg0 += ra.nsegg;
        u64* cur = nullptr;
        if (int rc = msm_reduce_windows(D, rb, ra, &cur)) return rc;
        // Horner's rule, top window first across the groups: this group continues from the result of the group above it
        // (same stream, or -- the lowest group -- behind that stream's event)
        if (g == G - 1 && G > 1 && ZC_MSM_TAIL_SIDE) HIP_TRY(hipStreamWaitEvent(st, D.ev_grp_done[G - 2], 0));
        // The lowest group's stretch of the rule is on the call's critical path: it takes the result of the groups above ALREADY
        // multiplied by 2^(c nw) -- k_msm_shift runs behind the second-lowest group's stretch on the side stream, beside the
        // lowest group's bucket sums (slot G of grp_out) -- and adds it last.
        const bool preshift = ZC_MSM_CARRY_PRESHIFT && G > 1 && ZC_MSM_TAIL_SIDE;
        const bool lowest = g == G - 1;
        const u64* carry = g == 0 ? nullptr : (lowest && preshift) ? grp_out + 20 * (size_t)G : grp_out + 20 * (size_t)(g - 1);
        hipLaunchKernelGGL(zc::k_msm_window_combine, dim3(1), dim3(64), 0, st, (const u64*)cur, grp_out + 20 * (size_t)g, ra.nw, c, carry, lowest && preshift ? 1 : 0);
        if (preshift && g == G - 2)
            hipLaunchKernelGGL(zc::k_msm_shift, dim3(1), dim3(64), 0, st, (const u64*)(grp_out + 20 * (size_t)g), grp_out + 20 * (size_t)G, c * mp.gw[G - 1]);
        if (st != D.s()) HIP_TRY(hipEventRecord(D.ev_grp_done[g], st));
    }
    *result = grp_out + 20 * (size_t)(G - 1);
    HIP_TRY(hipGetLastError());
    return ZC_OK;
}

// ---------------------------------------------------------------- RCCL (opened on demand)
RcclApi g_rccl;
std::mutex g_rccl_mu;

int rccl_load()
{
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    if (g_rccl.handle) return ZC_OK;
    // an RCCL already mapped by the host application (PyTorch ships one) is shared, not duplicated
    const char* names[] = {getenv("ZC_RCCL_PATH"), "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* nm : names)
        if (nm && !h) h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
    for (const char* nm : names)
        if (nm && !h) h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(ZC_ERR_HIP, "librccl.so not found (set ZC_RCCL_PATH)");
    RcclApi api;
    api.handle = h;
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
    api.CommCount = (decltype(api.CommCount))dlsym(h, "ncclCommCount");
    api.AllGather = (decltype(api.AllGather))dlsym(h, "ncclAllGather");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.CommCount || !api.AllGather || !api.GetErrorString)
        return fail(ZC_ERR_HIP, "librccl.so lacks an expected symbol");
    g_rccl = api;
    return ZC_OK;
}
int rccl_fail(const char* what, ncclResult_t r)
{
    g_last_error = std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error");
    return ZC_ERR_HIP;
}
#define RCCL_TRY(expr)                                         \
    do {                                                       \
        ncclResult_t r_ = (expr);                              \
        if (r_ != ncclSuccess) return rccl_fail(#expr, r_);    \
    } while (0)

// The inputs of an MSM call to device D, which becomes the current device; an asynchronous failure of an earlier windowed-core
// call surfaces here too.  Host arrays (on_device false) are uploaded on D.s() into D.scratch[0] (160-byte points) and
// D.scratch[1] (40-byte scalars) and the pointers redirected; a null array is skipped (zc_msm_fixed: the points are the table's).
int msm_stage(DevState& D, bool on_device, const u64** points, size_t npoints, const u64** scalars, size_t nscalars)
{
    if (int rc = ring_check(D)) return rc;
    HIP_TRY(hipSetDevice(D.device));
    if (on_device) return ZC_OK;
    const u64** const arr[2] = {points, scalars};
    const size_t bytes[2] = {npoints * 160, nscalars * 40};
    for (int a = 0; a < 2; a++)
        if (arr[a])
            if (int rc = D.scratch[a].grow(bytes[a])) return rc;
    for (int a = 0; a < 2; a++) {
        if (!arr[a]) continue;
        HIP_TRY(hipMemcpyAsync(D.scratch[a].as<void>(), *arr[a], bytes[a], hipMemcpyHostToDevice, D.s()));
        *arr[a] = D.scratch[a].as<const u64>();
    }
    return ZC_OK;
}

// One device's shard of an MSM, inputs host (staged) or device (in place); the 160-byte sum stays
// in device memory (*result), everything enqueued on ds.s().
int msm_shard(DevState& ds, const uint64_t* points, const uint64_t* scalars, size_t cnt, bool on_device, const u64** result)
{
    if (int rc = msm_stage(ds, on_device, &points, cnt, &scalars, cnt)) return rc;
    return msm_on_device(ds, points, scalars, cnt, result);
}

// ---------------------------------------------------------------- batched variable-base MSM (zc_msm_batch)
// The batch's sums (`batch` independent MSMs of n pairs each, instance-major), enqueued on D.s() without any host
// synchronisation: *result = batch canonical points in D.msm (valid until the next MSM on this device).  batch >= 2, n >= 1,
// limits checked.  The regimes and the window width: zc_msm_plan.h, msm_batch_plan.
int msm_batch_on_device(DevState& D, const u64* dP, const u64* dK, size_t n, size_t batch, const u64** result)
{
    const Tuning& tune = D.tune;
    const MsmBucketPlan bp = msm_batch_plan(n, batch, aligned16(dP), tune.msm);
    const size_t cnt = n * batch;
    if (!bp.buckets) {
        // two buffers of the workspace: the batch n products, and the other side of the folds' ping-pong
        const size_t prod_bytes = (cnt * 160 + 255) & ~(size_t)255, half_bytes = (batch * ((n + 1) / 2) * 160 + 255) & ~(size_t)255;
        if (int rc = D.msm.grow(prod_bytes + half_bytes)) return rc;
        u64* cur = D.msm.as<u64>();
        u64* nxt = (u64*)(D.msm.as<char>() + prod_bytes);
        scalar_mul_on_device(D, dP, dK, cur, cnt);
        // every level halves every row: rows of n, ceil(n / 2), ... points, ping-pong between the two buffers
        for (size_t len = n; len > 1; len = (len + 1) / 2) {
            hipLaunchKernelGGL(zc::k_msm_fold_rows, dim3(grid_for(batch * ((len + 1) / 2))), dim3(zc::ZC_BLOCK), 0, D.s(), (const u64*)cur, nxt, batch, len);
            std::swap(cur, nxt);
        }
        *result = cur;
        HIP_TRY(hipGetLastError());
        return ZC_OK;
    }
    const int c = bp.c, W = bp.W;
    MsmWorkspace ws;
    if (int rc = msm_workspace(D, bp, cnt, batch, &ws)) return rc;
    // one normalisation over all batch n points: it is per point, instance boundaries do not matter
    if (bp.affine)
        msm_prepare_affine(D.s(), dP, ws.cached, cnt, tune, (zc::u32)(bp.rec_bytes / 4));
    else
        hipLaunchKernelGGL(aligned16(dP) ? zc::k_msm_prepare : zc::k_msm_prepare_lane, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dP, ws.cached, cnt);
    hipLaunchKernelGGL(zc::k_msm_fixed_digits, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dK, ws.digits, n, batch, c, W);
    HIP_TRY(hipMemsetAsync(ws.present, 0, bp.nb, D.s()));
    if (int rc = msm_sort(D, D.s(), bp.sort, 0, (int)bp.nw, ws.digits, ws.pairs_a, ws.pairs_b, ws.sort_table, bp.sort.table_words, ws.sort_sums)) return rc;
    hipLaunchKernelGGL(zc::k_msm_batch_rebase, dim3(grid_for(bp.m)), dim3(zc::ZC_BLOCK), 0, D.s(), ws.pairs_a, bp.m, (zc::u32)bp.nb, (zc::u32)((size_t)W << (c - 1)), (zc::u32)n);
    u64* sums = nullptr;
    if (int rc = msm_reduce_windows(D, msm_reduce_bufs(bp, ws, ws.cached), msm_reduce_flat(bp, ws), &sums)) return rc;
    // Horner's rule over every instance's W window sums at once: 16 instances per 64-lane workgroup
    hipLaunchKernelGGL(zc::k_msm_window_combine_batch, dim3((unsigned)((batch + 15) / 16)), dim3(64), 0, D.s(), (const u64*)sums, ws.out, batch, W, c);
    *result = ws.out;
    HIP_TRY(hipGetLastError());
    return ZC_OK;
}

// The launch of an op with one inversion per element over the buffers p... in the form zc_launch_plan.h names (inversion_form):
// `k` with one element per lane, or the chunked kernel on lanes that share an inversion among c elements -- `k_lone` its
// independent-chain multiplier form.
template <class K, class KC, class... P>
int launch_shared_inversions(DevState& D, size_t cnt, bool in_place, K k, KC k_chunked, KC k_lone, P... p)
{
    const zc::InversionPlan ip = zc::inversion_form(cnt, in_place, D.tune.inv_chunk, D.cus);
    count_form(D, ip.form);
    if (ip.form == zc::FORM_INV_PER_ELEMENT)
        hipLaunchKernelGGL(k, dim3(grid_for(ip.lanes)), dim3(zc::ZC_BLOCK), 0, D.s(), p..., cnt);
    else
        hipLaunchKernelGGL(ip.form == zc::FORM_INV_LONE ? k_lone : k_chunked, dim3(grid_for(ip.lanes)), dim3(zc::ZC_BLOCK), 0, D.s(), p..., cnt, (int)ip.c);
    return ZC_OK;
}

const uint64_t IDENT_POINT[20] = {0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// The three SHA-512 calls (include/zerocaf_hip_ext_hash.h): the argument checks in the header's order, then run_batched over
// the parts and the output -- every part an ordinary buffer of part_len[j] bytes per row -- and one launch of `k` per piece with
// the prefix and the lengths in its argument block.  `out_name`: the output's parameter name, `out_per` elements of T per row.
template <class T>
int hash_rows_call(zc_ctx* ctx, void (*k)(const zc::HashMsg, T*, size_t), const uint8_t* prefix, size_t prefix_len, const uint8_t* const* parts,
                   const size_t* part_len, size_t nparts, T* out, const char* out_name, size_t out_per, size_t n)
{
    REQUIRE(parts);
    REQUIRE(part_len);
    if (!out) return failf(ZC_ERR_BAD_ARG, "null pointer: %s", out_name);
    if (prefix_len > 0) REQUIRE(prefix);
    if (nparts < 1 || nparts > (size_t)zc::HASH_MAX_PARTS) return failf(ZC_ERR_BAD_ARG, "nparts must be 1 .. %d", zc::HASH_MAX_PARTS);
    for (size_t j = 0; j < nparts; j++)
        if (!parts[j]) return failf(ZC_ERR_BAD_ARG, "null pointer: parts[%zu]", j);
    for (size_t j = 0; j < nparts; j++)
        if (part_len[j] == 0) return failf(ZC_ERR_BAD_ARG, "part_len[%zu] must be at least 1", j);
    if (prefix_len > zc::HASH_MAX_PREFIX) return failf(ZC_ERR_BAD_ARG, "prefix_len must be at most %u", zc::HASH_MAX_PREFIX);
    size_t total = prefix_len;
    for (size_t j = 0; j < nparts; j++) {
        if (part_len[j] > zc::HASH_MAX_ROW_BYTES - total) return failf(ZC_ERR_BAD_ARG, "a row (prefix_len + every part_len) must be at most %u bytes", zc::HASH_MAX_ROW_BYTES);
        total += part_len[j];
    }
    for (size_t j = 0; j < nparts; j++)
        if (n > SIZE_MAX / part_len[j]) return failf(ZC_ERR_BAD_ARG, "n * part_len[%zu] overflows size_t", j);
    if (n > SIZE_MAX / (sizeof(T) * out_per)) return failf(ZC_ERR_BAD_ARG, "n rows of %s overflow size_t", out_name);

    zc::HashMsg m = {};
    m.nparts = (zc::u32)nparts;
    m.prefix_len = (zc::u32)prefix_len;
    m.total = (zc::u32)total;
    if (prefix_len) memcpy(m.prefix, prefix, prefix_len);
    Arg args[MAX_ARGS];
    for (size_t j = 0; j < nparts; j++) {
        m.part_len[j] = (zc::u32)part_len[j];
        args[j] = Arg{parts[j], part_len[j], false};
    }
    args[nparts] = Arg{out, sizeof(T) * out_per, true};
    return run_batched(ctx, args, (int)nparts + 1, n, [&](void** d, size_t cnt, DevState& D) -> int {
        zc::HashMsg piece = m;
        unsigned mod8[zc::HASH_MAX_PARTS];
        for (size_t j = 0; j < nparts; j++) {
            piece.part[j] = static_cast<const uint8_t*>(d[j]);
            mod8[j] = (unsigned)(reinterpret_cast<uintptr_t>(d[j]) % 8);
        }
        piece.words = zc::hash_reader_words(prefix_len, part_len, mod8, nparts, D.tune.test_hash_bytes) ? 1 : 0;
        hipLaunchKernelGGL(k, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), piece, static_cast<T*>(d[nparts]), cnt);
        return ZC_OK;
    }, false);
}

// enqueue(what) -> status runs its steps on D's stream until the first failure; the stream is drained in either case, so that the
// staging blocks declared before this call outlive whatever was enqueued.  The first error wins: the status of `enqueue`, else
// the synchronisation's under `what`.
template <class F>
int enqueue_and_drain(DevState& D, const char* what, F&& enqueue)
{
    const int rc = enqueue(what);
    const hipError_t synced = hipStreamSynchronize(D.s());
    if (rc) return rc;
    return synced == hipSuccess ? ZC_OK : fail(ZC_ERR_HIP, what, synced);
}
// The one small input of a create call in host memory: copied, or -- device-resident -- brought down once on its owner's stream.
// `who` prefixes the messages about where the input lives.
int fetch_once(zc_ctx* ctx, const char* who, const void* src, void* host, size_t bytes)
{
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, {src}, who, &owner)) return rc;
    if (!owner) return memcpy(host, src, bytes), ZC_OK;
    HIP_TRY(hipSetDevice(owner->device));
    HIP_TRY(hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, owner->s()));
    HIP_TRY(hipStreamSynchronize(owner->s()));
    return ZC_OK;
}

// ---- the tables of a context by id: the member of the context that holds a kind, and what the calls of two kinds say about an
// id that is no live table of theirs
template <class T>
using TablesOf = Tables<T> zc_ctx::*;
constexpr const char* NO_GENS = "unknown generator set";
constexpr const char* NO_DLOG = "unknown dlog table";
// The table `id` names, with the context's lock held.  A row call's launch looks its table up with it a second time, under the lock
// the batched call holds (a table destroyed since the first look is refused), and takes mem[D.slot]: that happens on run_batched's
// worker threads too, while the calling thread holds the lock, so this only reads.
template <class T>
int table_find(zc_ctx* ctx, TablesOf<T> kind, uint64_t id, const char* unknown, T** t)
{
    *t = (ctx->*kind).find(id);
    return *t ? ZC_OK : fail(ZC_ERR_BAD_ARG, unknown);
}
// A row call's first look at its table, before its argument checks: facts(table) copies out what they need under a short lock.
template <class T, class F>
int table_facts(zc_ctx* ctx, TablesOf<T> kind, uint64_t id, const char* unknown, F&& facts)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    T* t = nullptr;
    if (int rc = table_find(ctx, kind, id, unknown, &t)) return rc;
    facts(*t);
    return ZC_OK;
}
// zc_msm_bases_destroy, zc_gens_destroy, zc_dlog_destroy: the stream of every slot on which the table holds memory is drained
// before any of that memory goes; slot 0's device is current afterwards, and a failing hipFree is reported (the table is gone then).
template <class T>
int table_destroy(zc_ctx* ctx, TablesOf<T> kind, uint64_t id, const char* unknown)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    T* t = nullptr;
    if (int rc = table_find(ctx, kind, id, unknown, &t)) return rc;
    for (DevState& D : ctx->devs) {                         // work that reads the table ends before it goes
        if (!t->mem[D.slot]) continue;
        HIP_TRY(hipSetDevice(D.device));
        HIP_TRY(hipStreamSynchronize(D.s()));
    }
    (void)hipSetDevice(ctx->devs[0].device);
    hipError_t freed = hipSuccess;
    for (DevBuf& b : t->mem)
        if (const hipError_t e = b.reset(); freed == hipSuccess) freed = e;
    (ctx->*kind).erase(id);
    HIP_TRY(freed);
    return ZC_OK;
}

// zc_ed_mul_gens and zc_ris_mul_gens_compress behind their pointer checks: the context, the id and n * count < 2^31 in the
// header's order, then one lane per row of `out_per` elements.
template <class OUT, class K>
int mul_gens(zc_ctx* ctx, uint64_t id, const uint64_t* scalars, OUT* out, size_t out_per, size_t n, const char* who, K kernel)
{
    size_t count = 0;
    if (int rc = table_facts(ctx, &zc_ctx::gens, id, NO_GENS, [&](const GenSet& g) { count = g.count; })) return rc;
    if (n >= ((size_t)1 << 31) / count + (((size_t)1 << 31) % count != 0)) return failf(ZC_ERR_BAD_ARG, "%s: n * count must stay below 2^31", who);
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* dk, OUT* dout) -> int {
        GenSet* g = nullptr;
        if (int rc = table_find(ctx, &zc_ctx::gens, id, NO_GENS, &g)) return rc;
        hipLaunchKernelGGL(kernel, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dk, dout, g->mem[D.slot].as<const zc::u32>(), (zc::u32)count, cnt);
        return ZC_OK;
    }, ROWS(scalars, 5 * count), ROWS(out, out_per));
}
// The launches of `cnt` rows of a point sum on slot D: one kernel, or -- more slices than a workgroup has lanes -- the first kernel into the
// slot's `sum` workspace and the one that finishes the rows, both on the slot's stream (a later call's kernels come behind them;
// a workspace that has to grow is freed first, which waits for the device).
template <class K1, class KP, class K2, class IN, class... OUT>
int sum_rows_launch(DevState& D, size_t cnt, size_t terms, K1 whole, KP part, K2 finish, const IN* in, OUT*... out)
{
    const zc::SumPlan p = zc::sum_plan(cnt, terms);
    if (p.grid1 >= ((size_t)1 << 31)) return fail(ZC_ERR_BAD_ARG, "more rows than one launch holds");       // rows without terms only: n * terms < 2^31 bounds every other grid
    if (p.form == zc::SUM_FORM_GROUP) {
        hipLaunchKernelGGL(whole, dim3((unsigned)p.grid1), dim3(zc::SUM_BLOCK), 0, D.s(), in, (zc::u32)terms, (zc::u32)p.parts, out..., cnt);
        return ZC_OK;
    }
    if (int rc = D.sum.grow(p.workspace_bytes)) return rc;
    zc::u32* const ws = D.sum.as<zc::u32>();
    hipLaunchKernelGGL(part, dim3((unsigned)p.grid1), dim3(zc::SUM_BLOCK), 0, D.s(), in, (zc::u32)terms, (zc::u32)p.parts, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(finish, dim3((unsigned)p.grid2), dim3(zc::SUM_BLOCK), 0, D.s(), (const zc::u32*)ws, (zc::u32)p.blocks_per_row, out..., cnt);
    return ZC_OK;
}
// The launches of `cnt` rows of a bounded discrete log on slot D, all on its stream: the slices of zc_dlog_plan.h, launch k from
// the offset W_k.
template <class K, class IN>
int dlog_launches_on(zc_ctx* ctx, uint64_t id, DevState& D, K kernel, const IN* in, uint64_t bound, u64* m_out, uint8_t* found, uint8_t* ok, size_t cnt)
{
    DlogTable* table = nullptr;
    if (int rc = table_find(ctx, &zc_ctx::dlogs, id, NO_DLOG, &table)) return rc;
    const DlogTable& tb = *table;
    const u64* const records = tb.mem[D.slot].as<const u64>();
    zc::dlog_launch A;
    A.table = zc::dlog_table{records, records + 4 * zc::dlog_records(tb.t), (zc::u32)tb.t};
    A.coset4 = (tb.flags & ZC_DLOG_COSET4) ? 1u : 0u;
    A.bound = bound;
    static_assert(sizeof(zc::dlog_step) == 27 * sizeof(zc::u32), "a cached affine point is 27 consecutive words of the setup block");
    memcpy(&A.S, tb.setup.data() + zc::DLOG_SETUP_STRIDE * zc::DLOG_SETUP_S, sizeof A.S);
    const unsigned grid = (unsigned)((cnt + zc::DLOG_BLOCK - 1) / zc::DLOG_BLOCK);
    for (uint64_t k = 0; k < zc::dlog_launches(bound, tb.t); k++) {
        const zc::DlogSlice s = zc::dlog_slice(bound, tb.t, k);
        A.launch = (zc::u32)k;
        A.first = s.first;
        A.chunks = s.chunks;
        memcpy(&A.W, tb.setup.data() + zc::dlog_offset_word(k), sizeof A.W);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(zc::DLOG_BLOCK), 0, D.s(), in, m_out, found, ok, A, cnt);
        HIP_TRY(hipGetLastError());
    }
    return ZC_OK;
}

}  // namespace

// =============================================================================== C ABI
extern "C" {

// ZC_SRC_HASH: sha256 of the kernel sources + the ABI header, passed in by dusk_zerocaf_amd/build.py;
// it ties a profile (profiles/roofline_inputs.json) to the build it was taken on
#ifndef ZC_SRC_HASH
#define ZC_SRC_HASH "unknown"
#endif
const char* zc_version(void) { return "zerocaf_hip 0.6 (gfx950, radix-2^29 Montgomery R=2^261) src:" ZC_SRC_HASH; }
const char* zc_last_error(void) { return g_last_error.c_str(); }

int zc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int zc_ctx_create(const int* devices, int ndev, zc_ctx** out)
{
    if (!out) return fail(ZC_ERR_BAD_ARG, "null out");
    *out = nullptr;
    int avail = zc_device_count();
    if (avail <= 0) return fail(ZC_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    std::vector<int> ids;
    if (!devices || ndev <= 0) {
        int cur = 0;
        HIP_TRY(hipGetDevice(&cur));
        ids.push_back(cur);
    } else {
        for (int i = 0; i < ndev; i++) {
            if (devices[i] < 0 || devices[i] >= avail) return fail(ZC_ERR_BAD_ARG, "device index out of range");
            ids.push_back(devices[i]);
        }
    }
    std::unique_ptr<zc_ctx> ctx(new zc_ctx());                // a failing step below releases what the steps before it created
    const Tuning tune = tuning_from_env();                   // the only place the library reads its knobs
    ctx->devs.reserve(ids.size());                           // the slots never move: pointers to them are taken everywhere
    for (int id : ids) {
        ctx->devs.emplace_back();
        const hipError_t e = ctx->devs.back().open(ctx->devs.size() - 1, id, tune);
        if (e != hipSuccess) return fail(ZC_ERR_HIP, "stream creation", e);
    }
    (void)hipSetDevice(ids[0]);
    *out = ctx.release();
    return ZC_OK;
}

int zc_ctx_device(zc_ctx* ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= (int)ctx->devs.size()) return fail(ZC_ERR_BAD_ARG, "zc_ctx_device: no such device slot");
    return ctx->devs[(size_t)slot].device;
}
int zc_ctx_device_count(zc_ctx* ctx) { return ctx ? (int)ctx->devs.size() : fail(ZC_ERR_BAD_ARG, "null context"); }

// Every slot drains its streams and releases what it holds (~DevState), then the tables of all kinds go.
int zc_ctx_destroy(zc_ctx* ctx)
{
    if (!ctx) return ZC_OK;
    if (ctx->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->comm);
    delete ctx;
    return ZC_OK;
}

// Switching the launch stream of a device slot: everything already enqueued on the old stream
// (including the producers of shared scratch: window tables, MSM workspace, the basepoint table)
// is ordered before later work on the new one with an event, without a host synchronisation.
int zc_ctx_set_stream_dev(zc_ctx* ctx, int slot, void* hip_stream, int external)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (slot < 0 || (size_t)slot >= ctx->devs.size()) return fail(ZC_ERR_BAD_ARG, "device slot out of range");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState& ds = ctx->devs[slot];
    hipStream_t next = external ? (hipStream_t)hip_stream : ds.stream;
    if (ds.s() == next && ds.use_borrowed == (external != 0)) return ZC_OK;
    HIP_TRY(hipSetDevice(ds.device));
    HIP_TRY(hipEventRecord(ds.ev_order, ds.s()));
    HIP_TRY(hipStreamWaitEvent(next, ds.ev_order, 0));
    ds.borrowed = external ? (hipStream_t)hip_stream : nullptr;
    ds.use_borrowed = external != 0;
    return ZC_OK;
}
int zc_ctx_set_stream(zc_ctx* ctx, void* hip_stream, int external) { return zc_ctx_set_stream_dev(ctx, 0, hip_stream, external); }

// Pin a caller-owned host buffer (hipHostRegister): copies from / to it are truly asynchronous
// and skip the runtime's bounce buffers.  Worth it for buffers reused across calls.
int zc_host_register(void* ptr, size_t bytes)
{
    if (!ptr || !bytes) return fail(ZC_ERR_BAD_ARG, "zc_host_register: null buffer");
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return ZC_OK;
}
int zc_host_unregister(void* ptr)
{
    if (!ptr) return fail(ZC_ERR_BAD_ARG, "zc_host_unregister: null buffer");
    HIP_TRY(hipHostUnregister(ptr));
    return ZC_OK;
}

// Waits for every slot's stream and reports the ring's error word.  The caller holds ctx->mu.
static int drain_slots_locked(zc_ctx* ctx)
{
    for (auto& ds : ctx->devs) {
        HIP_TRY(hipSetDevice(ds.device));
        HIP_TRY(hipStreamSynchronize(ds.s()));
        const int rc = ring_check(ds);
        if (rc) return rc;
    }
    return ZC_OK;
}

// Another thread may switch a slot's stream meanwhile (zc_ctx_set_stream_dev), so the handles are read under the lock.  The
// wait itself runs outside it: launches of other threads go on, and whatever was enqueued on a slot before this call -- on
// the stream it has now or, through the switch event, on an earlier one -- has completed when the wait returns.
int zc_ctx_synchronize(zc_ctx* ctx)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    std::vector<std::pair<int, hipStream_t>> streams;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        for (auto& ds : ctx->devs) streams.emplace_back(ds.device, ds.s());
    }
    for (auto& [device, stream] : streams) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    for (auto& ds : ctx->devs)
        if (const int rc = ring_check(ds)) return rc;
    return ZC_OK;
}

// ---- FieldElement
int zc_fe_add(zc_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) { return binop(c, zc::k_fe_add, a, b, o, n, 5, {zc::k_fe_add_stream}); }
int zc_fe_sub(zc_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) { return binop(c, zc::k_fe_sub, a, b, o, n, 5, {zc::k_fe_sub_stream}); }
// Mul / Square: LDS-staged beyond the Infinity Cache since round 5 -- with the one-pass product (151 / 115 multiply-adds instead of
// 270 / 234) the staged kernels' coalesced traffic pays: 2^24 elements, same box, mul 0.411 -> 0.376 ms, square 0.273 -> 0.248
// (with the two Montgomery passes of rounds 1-4 the staged kernels were the slower ones: 0.435 against 0.360 ms).
#ifndef ZC_MULSQ_STAGED
#define ZC_MULSQ_STAGED 1            // 0: A/B build with per-lane accesses at every size
#endif
#ifndef ZC_MULSQ_STAGED_MIN_BYTES
#define ZC_MULSQ_STAGED_MIN_BYTES zc::STREAM_BYTES
#endif
// Neg: one input array, no arithmetic to speak of.  Round 6 A/B at 2^24 / 2^26 decides whether the staged form ships
// (profiles/r06_experiments/neg_staged_ab.md); a kernel without a launch site is not kept.
#ifndef ZC_NEG_STAGED
#define ZC_NEG_STAGED 1
#endif
int zc_fe_mul(zc_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) { return binop(c, zc::k_fe_mul, a, b, o, n, 5, {ZC_MULSQ_STAGED ? zc::k_fe_mul_stream : nullptr, {ZC_MULSQ_STAGED_MIN_BYTES}}); }
int zc_fe_neg(zc_ctx* c, const uint64_t* a, uint64_t* o, size_t n) { return unop(c, zc::k_fe_neg, a, o, n, 5, {ZC_NEG_STAGED ? zc::k_fe_neg_stream : nullptr}); }
int zc_fe_square(zc_ctx* c, const uint64_t* a, uint64_t* o, size_t n) { return unop(c, zc::k_fe_square, a, o, n, 5, {ZC_MULSQ_STAGED ? zc::k_fe_square_stream : nullptr, {ZC_MULSQ_STAGED_MIN_BYTES}}); }

int zc_fe_invert(zc_ctx* ctx, const uint64_t* a, uint64_t* out, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* da, u64* dout, uint8_t* dok) {
        return launch_shared_inversions(D, cnt, dout == da, zc::k_fe_invert, zc::k_fe_invert_chunked, zc::k_fe_invert_chunked_lone, da, dout, dok);
    }, ROWS(a, 5), ROWS(out, 5), OPT_ROWS(ok, 1));
}
int zc_fe_div(zc_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* da, const u64* db, u64* dout, uint8_t* dok) {
        return launch_shared_inversions(D, cnt, dout == da || dout == db, zc::k_fe_div, zc::k_fe_div_chunked, zc::k_fe_div_chunked_lone, da, db, dout, dok);
    }, ROWS(a, 5), ROWS(b, 5), ROWS(out, 5), OPT_ROWS(ok, 1));
}
int zc_fe_half(zc_ctx* c, const uint64_t* a, uint64_t* o, size_t n) { return unop(c, zc::k_fe_half, a, o, n, 5); }
int zc_fe_pow(zc_ctx* c, const uint64_t* a, const uint64_t* e, uint64_t* o, size_t n) { return binop(c, zc::k_fe_pow, a, e, o, n, 5); }
// ZC_JACOBI_ROUNDS=r (tests): rounds of 30 positive division steps before a lane falls back to the exponentiation
int zc_fe_legendre_symbol(zc_ctx* ctx, const uint64_t* a, uint8_t* out, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* da, uint8_t* dout) {
        hipLaunchKernelGGL(zc::k_fe_legendre, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), da, dout, cnt, D.tune.jacobi_rounds >= 0 ? D.tune.jacobi_rounds : zc::JACOBI_MAX_ROUNDS);
        return ZC_OK;
    }, ROWS(a, 5), ROWS(out, 1));
}
int zc_fe_is_positive(zc_ctx* ctx, const uint64_t* a, uint8_t* out, size_t n) { return batched(ctx, n, false, plain(zc::k_fe_is_positive), ROWS(a, 5), ROWS(out, 1)); }
int zc_fe_mod_sqrt(zc_ctx* ctx, const uint64_t* a, int sign, uint64_t* out, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, u64* dout, uint8_t* dok) {
        hipLaunchKernelGGL(zc::k_fe_mod_sqrt, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), da, sign, dout, dok, cnt);
        return ZC_OK;
    }, ROWS(a, 5), ROWS(out, 5), OPT_ROWS(ok, 1));
}
// k_from_bytes serves both codecs: the field's takes every 32 bytes (no mask), the scalar's rejects what is not below the order
static int from_bytes(zc_ctx* ctx, const uint8_t* in32, uint64_t* out, uint8_t* ok, int is_scalar, size_t n)
{
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const uint8_t* din, u64* dout, uint8_t* dok) {
        hipLaunchKernelGGL(zc::k_from_bytes, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), din, dout, dok, is_scalar, cnt);
        return ZC_OK;
    }, ROWS(in32, 32), ROWS(out, 5), OPT_ROWS(ok, 1));
}
int zc_fe_from_bytes(zc_ctx* ctx, const uint8_t* in32, uint64_t* out, size_t n) { return from_bytes(ctx, in32, out, nullptr, 0, n); }
int zc_fe_to_bytes(zc_ctx* ctx, const uint64_t* in, uint8_t* out32, size_t n) { return batched(ctx, n, false, plain(zc::k_to_bytes), ROWS(in, 5), ROWS(out32, 32)); }
int zc_fe_sqrt_ratio_i(zc_ctx* ctx, const uint64_t* u, const uint64_t* v, uint64_t* out, uint8_t* was_square, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_fe_sqrt_ratio_i), ROWS(u, 5), ROWS(v, 5), ROWS(out, 5), OPT_ROWS(was_square, 1));
}
int zc_fe_inv_sqrt(zc_ctx* ctx, const uint64_t* a, uint64_t* out, uint8_t* was_square, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_fe_inv_sqrt), ROWS(a, 5), ROWS(out, 5), OPT_ROWS(was_square, 1));
}

// ---- Scalar
int zc_sc_add(zc_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) { return binop(c, zc::k_sc_add, a, b, o, n, 5, {zc::k_sc_add_stream}); }
int zc_sc_sub(zc_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) { return binop(c, zc::k_sc_sub, a, b, o, n, 5, {zc::k_sc_sub_stream}); }
int zc_sc_mul(zc_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* o, size_t n) { return binop(c, zc::k_sc_mul, a, b, o, n, 5, {ZC_MULSQ_STAGED ? zc::k_sc_mul_stream : nullptr, {ZC_MULSQ_STAGED_MIN_BYTES}}); }
int zc_sc_neg(zc_ctx* c, const uint64_t* a, uint64_t* o, size_t n) { return unop(c, zc::k_sc_neg, a, o, n, 5, {ZC_NEG_STAGED ? zc::k_sc_neg_stream : nullptr}); }
int zc_sc_square(zc_ctx* c, const uint64_t* a, uint64_t* o, size_t n) { return unop(c, zc::k_sc_square, a, o, n, 5, {ZC_MULSQ_STAGED ? zc::k_sc_square_stream : nullptr, {ZC_MULSQ_STAGED_MIN_BYTES}}); }
// S-x rows: the Scalar operations beside the default scalar-mul path
int zc_sc_half(zc_ctx* c, const uint64_t* a, uint64_t* o, size_t n) { return unop(c, zc::k_sc_half, a, o, n, 5); }
int zc_sc_pow(zc_ctx* c, const uint64_t* a, const uint64_t* e, uint64_t* o, size_t n) { return binop(c, zc::k_sc_pow, a, e, o, n, 5); }
int zc_sc_shr(zc_ctx* ctx, const uint64_t* a, unsigned shift, uint64_t* out, size_t n)
{
    if (shift > 255) return fail(ZC_ERR_BAD_ARG, "zc_sc_shr: the reference shifts by a u8");
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, u64* dout) {
        hipLaunchKernelGGL(zc::k_sc_shr, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), da, (zc::u32)shift, dout, cnt);
        return ZC_OK;
    }, ROWS(a, 5), ROWS(out, 5));
}
int zc_sc_into_bits(zc_ctx* ctx, const uint64_t* a, uint8_t* bits256, size_t n) { return batched(ctx, n, false, plain(zc::k_sc_into_bits), ROWS(a, 5), ROWS(bits256, 256)); }
int zc_sc_compute_naf(zc_ctx* ctx, const uint64_t* a, unsigned width, int8_t* naf256, size_t n)
{
    if (width == 1 || width > 7) return fail(ZC_ERR_BAD_ARG, "zc_sc_compute_naf: width 0 (compute_NAF) or 2..7 (compute_window_NAF: digits are i8)");
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, int8_t* dnaf) {
        hipLaunchKernelGGL(zc::k_sc_compute_naf, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), da, (zc::u32)width, dnaf, cnt);
        return ZC_OK;
    }, ROWS(a, 5), ROWS(naf256, 256));
}
int zc_sc_from_bytes(zc_ctx* ctx, const uint8_t* in32, uint64_t* out, uint8_t* ok, size_t n) { return from_bytes(ctx, in32, out, ok, 1, n); }
int zc_sc_to_bytes(zc_ctx* ctx, const uint64_t* in, uint8_t* out32, size_t n) { return zc_fe_to_bytes(ctx, in, out32, n); }
// ---- Scalar operations for protocols (not in the reference): reduction of 64 / 32 arbitrary bytes, a b + c, a^-1 mod L
int zc_sc_from_bytes_wide(zc_ctx* ctx, const uint8_t* in64, uint64_t* out, size_t n) { return batched(ctx, n, false, plain(zc::k_sc_from_bytes_wide), ROWS(in64, 64), ROWS(out, 5)); }
int zc_sc_from_bytes_mod_order(zc_ctx* ctx, const uint8_t* in32, uint64_t* out, size_t n) { return batched(ctx, n, false, plain(zc::k_sc_from_bytes_mod_order), ROWS(in32, 32), ROWS(out, 5)); }
int zc_sc_muladd(zc_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_sc_muladd), ROWS(a, 5), ROWS(b, 5), ROWS(c, 5), ROWS(out, 5));
}
int zc_sc_invert(zc_ctx* ctx, const uint64_t* a, uint64_t* out, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* da, u64* dout, uint8_t* dok) {
        return launch_shared_inversions(D, cnt, dout == da, zc::k_sc_invert, zc::k_sc_invert_chunked, zc::k_sc_invert_chunked_lone, da, dout, dok);
    }, ROWS(a, 5), ROWS(out, 5), OPT_ROWS(ok, 1));
}

// ---- EdwardsPoint
// staged records above 2^12 points (zc_launch_plan.h: ED_STAGED_MIN_POINTS)
int zc_ed_add(zc_ctx* c, const uint64_t* p, const uint64_t* q, uint64_t* o, size_t n) { return binop(c, zc::k_ed_add, p, q, o, n, 20, staged_points(zc::k_ed_add_staged)); }
int zc_ed_sub(zc_ctx* c, const uint64_t* p, const uint64_t* q, uint64_t* o, size_t n) { return binop(c, zc::k_ed_sub, p, q, o, n, 20, staged_points(zc::k_ed_sub_staged)); }
int zc_ed_double(zc_ctx* c, const uint64_t* p, uint64_t* o, size_t n) { return unop(c, zc::k_ed_double, p, o, n, 20, staged_points(zc::k_ed_double_staged)); }
int zc_ed_neg(zc_ctx* c, const uint64_t* p, uint64_t* o, size_t n) { return unop(c, zc::k_ed_neg, p, o, n, 20, staged_points(zc::k_ed_neg_staged)); }

// the reference's other scalar multiplications, one lane per row: (point, scalar) -> point, a long-running kernel
static int scalar_mul_variant(zc_ctx* ctx, kbin_t k, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n)
{
    return batched(ctx, n, true, plain(k), ROWS(a, 20), ROWS(b, 5), ROWS(out, 20));
}
int zc_ed_scalar_mul(zc_ctx* ctx, const uint64_t* p, const uint64_t* k, uint64_t* out, size_t n, unsigned flags)
{
    if (flags == ZC_SCALAR_MUL_STRICT) return scalar_mul_impl(ctx, p, k, out, n);
    if (flags == ZC_SCALAR_MUL_FAST)
        return batched(ctx, n, true, [](DevState& D, size_t cnt, const u64* dp, const u64* dk, u64* dout) {
            return fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
                hipLaunchKernelGGL(zc::k_ed_scalar_mul_fast, dim3(grid_for(c)), dim3(zc::ZC_BLOCK), 0, D.s(), dp + 20 * off, dk + 5 * off, (zc::u32)5, dout + 20 * off,
                                   table, ring, slots, (zc::u32)c);
            });
        }, ROWS(p, 20), ROWS(k, 5), ROWS(out, 20));
    if (flags == ZC_SCALAR_MUL_LTR_BIN) return scalar_mul_variant(ctx, zc::k_ed_scalar_mul_ltr_bin, p, k, out, n);
    if (flags == ZC_SCALAR_MUL_BINARY_NAF) return scalar_mul_variant(ctx, zc::k_ed_scalar_mul_naf, p, k, out, n);
    return fail(ZC_ERR_BAD_ARG, "unknown scalar_mul flags");
}
// out[i] = sum_j k[i][j] * P[i][j]: one shared doubling chain per row (zc_curve.hip.h: lincomb_fast)
int zc_ed_lincomb(zc_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t terms, uint64_t* out, size_t n)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (terms < 1 || terms > ZC_LINCOMB_MAX_TERMS) return fail(ZC_ERR_BAD_ARG, "zc_ed_lincomb: terms must be 1..ZC_LINCOMB_MAX_TERMS");
    if (n >= ((size_t)1 << 31) / terms + (((size_t)1 << 31) % terms != 0)) return fail(ZC_ERR_BAD_ARG, "zc_ed_lincomb: n * terms must stay below 2^31");
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const u64* dp, const u64* dk, u64* dout) -> int {
        const zc::LincombLaunch ll = zc::lincomb_launch(terms);
        const zc::u32 units = (zc::u32)zc::ring_units_per_xcd(terms);
        if (int rc = fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
                hipLaunchKernelGGL(zc::k_ed_lincomb, dim3((unsigned)((c + ll.block - 1) / ll.block)), dim3(ll.block), ll.lds_bytes, D.s(),
                                   dp + 20 * terms * off, dk + 5 * terms * off, (zc::u32)terms, dout + 20 * off, table, ring, slots, units, (zc::u32)terms, (zc::u32)c);
            }, terms))
            return rc;
        hipLaunchKernelGGL(zc::k_ed_lincomb_off_curve_rows, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dp, dk, (zc::u32)terms, dout, (zc::u32)cnt);
        return ZC_OK;
    }, ROWS(points, 20 * terms), ROWS(scalars, 5 * terms), ROWS(out, 20));
}
int zc_ed_mul_by_pow_2(zc_ctx* ctx, const uint64_t* p, uint64_t kexp, uint64_t* out, size_t n)
{
    if (kexp >= 250) return fail(ZC_ERR_BAD_ARG, "Exponent can't be greater than the sub-group order");   // scalar.rs:531
    uint64_t k[5] = {0, 0, 0, 0, 0};
    k[kexp / 52] = 1ull << (kexp % 52);                  // Scalar::two_pow_k, scalar.rs:525-552
    return scalar_mul_bcast(ctx, p, k, out, n);
}
int zc_ed_mul_by_cofactor(zc_ctx* ctx, const uint64_t* p, uint64_t* out, size_t n)
{
    return zc_ed_mul_by_pow_2(ctx, p, 3, out, n);         // Scalar::from(8u8), edwards.rs:174-179
}
int zc_ed_to_affine(zc_ctx* ctx, const uint64_t* p, uint64_t* xy, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* dp, u64* dxy, uint8_t* dok) {
        // (one chunked kernel at every size, and a 160-byte row cannot be normalised in place)
        return launch_shared_inversions(D, cnt, false, zc::k_ed_to_affine, zc::k_ed_to_affine_chunked, zc::k_ed_to_affine_chunked, dp, dxy, dok);
    }, ROWS(p, 20), ROWS(xy, 10), OPT_ROWS(ok, 1));
}
int zc_ed_eq(zc_ctx* ctx, const uint64_t* p, const uint64_t* q, uint8_t* eq, size_t n) { return batched(ctx, n, false, plain(zc::k_ed_eq), ROWS(p, 20), ROWS(q, 20), ROWS(eq, 1)); }
int zc_ed_compress(zc_ctx* ctx, const uint64_t* p, uint8_t* out32, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_ed_compress), ROWS(p, 20), ROWS(out32, 32), OPT_ROWS(ok, 1));
}
int zc_ed_decompress(zc_ctx* ctx, const uint8_t* in32, uint64_t* out, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_ed_decompress), ROWS(in32, 32), ROWS(out, 20), OPT_ROWS(ok, 1));
}

// ---- Ristretto
int zc_ris_compress(zc_ctx* ctx, const uint64_t* p, uint8_t* out32, size_t n) { return batched(ctx, n, false, plain(zc::k_ris_compress), ROWS(p, 20), ROWS(out32, 32)); }
int zc_ris_decompress(zc_ctx* ctx, const uint8_t* in32, uint64_t* out, uint8_t* ok, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_ris_decompress), ROWS(in32, 32), ROWS(out, 20), OPT_ROWS(ok, 1));
}
int zc_ris_eq(zc_ctx* ctx, const uint64_t* p, const uint64_t* q, uint8_t* eq, size_t n) { return batched(ctx, n, false, plain(zc::k_ris_eq), ROWS(p, 20), ROWS(q, 20), ROWS(eq, 1)); }
// zerocaf_hip_ext.h: the encodings of 2 P, one shared inversion per lane instead of a square root per row (zc_ris_batch.hip.h)
int zc_ris_double_and_compress(zc_ctx* ctx, const uint64_t* p, uint8_t* out32, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* dp, uint8_t* dout) {
        // (a 160-byte row cannot be encoded in place; the prefix products wait in the output rows themselves)
        return launch_shared_inversions(D, cnt, false, zc::k_ris_double_compress, zc::k_ris_double_compress_chunked, zc::k_ris_double_compress_chunked_lone, dp, dout);
    }, ROWS(p, 20), ROWS(out32, 32));
}
int zc_ris_roundtrip_mul(zc_ctx* ctx, const uint8_t* in32, const uint64_t* k, uint8_t* out32, uint8_t* ok, size_t n)
{
    // The boundary is encodings in / encodings out, which depend only on the group element, so
    // the fast scalar-mul core is used (ZC_RISTRETTO_STRICT=1 runs the reference formula sequence).
    return batched(ctx, n, true, [](DevState& D, size_t cnt, const uint8_t* din, const u64* dk, uint8_t* dout, uint8_t* dok) {
        if (D.tune.ristretto_strict) return plain(zc::k_ris_roundtrip_mul)(D, cnt, din, dk, dout, dok);
        return fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
            hipLaunchKernelGGL(zc::k_ris_roundtrip_mul_fast, dim3(grid_for(c)), dim3(zc::ZC_BLOCK), 0, D.s(), din + 32 * off, dk + 5 * off, dout + 32 * off,
                               dok ? dok + off : nullptr, table, ring, slots, (zc::u32)c);
        });
    }, ROWS(in32, 32), ROWS(k, 5), ROWS(out32, 32), OPT_ROWS(ok, 1));
}

// ---- one scalar for the whole batch (zerocaf_hip_ext_shared.h; kernels: zc_shared.hip.h, the host's recoding: zc_shared_scalar.h)
// k is read here, before anything is queued: what travels to the device is the schedule, by value in the kernel arguments.
static int shared_scalar_on_host(const uint64_t* k)
{
    Residency r = RES_HOST;
    int d = -1;
    residency_of(k, &r, &d);
    if (r == RES_DEVICE) return fail(ZC_ERR_BAD_ARG, "k must be host memory");
    return ZC_OK;
}
int zc_ed_scalar_mul_shared(zc_ctx* ctx, const uint64_t* p, const uint64_t* k, uint64_t* out, size_t n)
{
    REQUIRE(p);
    REQUIRE(k);
    REQUIRE(out);
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (n == 0) return ZC_OK;
    if (int rc = shared_scalar_on_host(k)) return rc;
    const zc::shared_schedule sched = zc::shared_schedule_ed(k);
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const u64* dp, u64* dout) {
        return fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
            hipLaunchKernelGGL(zc::k_ed_scalar_mul_shared, dim3(grid_for(c)), dim3(zc::ZC_BLOCK), 0, D.s(), dp + 20 * off, sched, dout + 20 * off, table, ring, slots, (zc::u32)c);
        });
    }, ROWS(p, 20), ROWS(out, 20));
}
int zc_ris_mul_shared(zc_ctx* ctx, const uint8_t* in32, const uint64_t* k, uint8_t* out32, uint8_t* ok, size_t n)
{
    REQUIRE(in32);
    REQUIRE(k);
    REQUIRE(out32);
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (n == 0) return ZC_OK;
    if (int rc = shared_scalar_on_host(k)) return rc;
    const zc::shared_schedule sched = zc::shared_schedule_wire(k);          // of k' = (k mod L) / 2 mod L: the kernel encodes 2 (k' P)
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const uint8_t* din, uint8_t* dout, uint8_t* dok) {
        return fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
            hipLaunchKernelGGL(zc::k_ris_mul_shared, dim3(grid_for(c)), dim3(zc::ZC_BLOCK), 0, D.s(), din + 32 * off, sched, dout + 32 * off, dok ? dok + off : nullptr,
                               table, ring, slots, (zc::u32)c);
        });
    }, ROWS(in32, 32), ROWS(out32, 32), OPT_ROWS(ok, 1));
}
// ---- one scalar VECTOR for the whole batch (zerocaf_hip_ext_shared_lincomb.h): out[i] = sum_j k_j * P_ij.  The terms' recodings
// are merged into one schedule here (zc_shared_scalar.h: shared_lincomb_schedule), which travels by value like the single
// scalar's.  Ring geometry is zc_ed_lincomb's (one 64 KB unit per term and wave slot); the kernels keep no digits in LDS, so
// every term count runs 256-lane workgroups without dynamic LDS.
static int shared_lincomb_args(const char* who, size_t terms, size_t n)
{
    if (terms < 1 || terms > ZC_LINCOMB_MAX_TERMS) return failf(ZC_ERR_BAD_ARG, "%s: terms must be 1..ZC_LINCOMB_MAX_TERMS", who);
    if (n >= ((size_t)1 << 31) / terms + (((size_t)1 << 31) % terms != 0)) return failf(ZC_ERR_BAD_ARG, "%s: n * terms must stay below 2^31", who);
    return ZC_OK;
}
int zc_ed_lincomb_shared(zc_ctx* ctx, const uint64_t* points, const uint64_t* k, size_t terms, uint64_t* out, size_t n)
{
    REQUIRE(points);
    REQUIRE(k);
    REQUIRE(out);
    if (int rc = shared_lincomb_args("zc_ed_lincomb_shared", terms, n)) return rc;
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (n == 0) return ZC_OK;
    if (int rc = shared_scalar_on_host(k)) return rc;
    const zc::shared_lincomb_schedule sched = zc::shared_lincomb_schedule_ed(k, terms);
    const zc::u32 units = (zc::u32)zc::ring_units_per_xcd(terms);
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const u64* dp, u64* dout) {
        return fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
            hipLaunchKernelGGL(zc::k_ed_lincomb_shared, dim3(grid_for(c)), dim3(zc::ZC_BLOCK), 0, D.s(), dp + 20 * terms * off, sched, dout + 20 * off, table, ring, slots,
                               units, (zc::u32)c);
        }, terms);
    }, ROWS(points, 20 * terms), ROWS(out, 20));
}
int zc_ris_lincomb_shared(zc_ctx* ctx, const uint8_t* in32, const uint64_t* k, size_t terms, uint8_t* out32, uint8_t* ok, size_t n)
{
    REQUIRE(in32);
    REQUIRE(k);
    REQUIRE(out32);
    if (int rc = shared_lincomb_args("zc_ris_lincomb_shared", terms, n)) return rc;
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (n == 0) return ZC_OK;
    if (int rc = shared_scalar_on_host(k)) return rc;
    const zc::shared_lincomb_schedule sched = zc::shared_lincomb_schedule_wire(k, terms);    // of the k'_j: the kernel encodes 2 (sum k'_j P_j)
    const zc::u32 units = (zc::u32)zc::ring_units_per_xcd(terms);
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const uint8_t* din, uint8_t* dout, uint8_t* dok) {
        return fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
            hipLaunchKernelGGL(zc::k_ris_lincomb_shared, dim3(grid_for(c)), dim3(zc::ZC_BLOCK), 0, D.s(), din + 32 * terms * off, sched, dout + 32 * off,
                               dok ? dok + off : nullptr, table, ring, slots, units, (zc::u32)c);
        }, terms);
    }, ROWS(in32, 32 * terms), ROWS(out32, 32), OPT_ROWS(ok, 1));
}

// ---- "next" rows (N3, N4)
int zc_ed_is_valid(zc_ctx* ctx, const uint64_t* p, uint8_t* valid, size_t n) { return batched(ctx, n, false, plain(zc::k_ed_is_valid), ROWS(p, 20), ROWS(valid, 1)); }
int zc_ris_is_valid(zc_ctx* ctx, const uint64_t* p, uint8_t* valid, size_t n) { return batched(ctx, n, false, plain(zc::k_ris_is_valid), ROWS(p, 20), ROWS(valid, 1)); }
int zc_ris_elligator(zc_ctx* ctx, const uint64_t* r0, uint64_t* out, size_t n) { return batched(ctx, n, false, plain(zc::k_ris_elligator), ROWS(r0, 5), ROWS(out, 20)); }
int zc_ris_from_uniform_bytes(zc_ctx* ctx, const uint8_t* in64, uint64_t* out, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_ris_from_uniform_bytes), ROWS(in64, 64), ROWS(out, 20));
}
// ---- SHA-512 over batched rows (zerocaf_hip_ext_hash.h): the digest, and the two calls above fused behind it
int zc_sha512_rows(zc_ctx* ctx, const uint8_t* prefix, size_t prefix_len, const uint8_t* const* parts, const size_t* part_len, size_t nparts, uint8_t* out64, size_t n)
{
    return hash_rows_call(ctx, zc::k_sha512_rows, prefix, prefix_len, parts, part_len, nparts, out64, "out64", 64, n);
}
int zc_sc_from_sha512(zc_ctx* ctx, const uint8_t* prefix, size_t prefix_len, const uint8_t* const* parts, const size_t* part_len, size_t nparts, uint64_t* out, size_t n)
{
    return hash_rows_call(ctx, zc::k_sc_from_sha512, prefix, prefix_len, parts, part_len, nparts, out, "out", 5, n);
}
int zc_ris_from_sha512(zc_ctx* ctx, const uint8_t* prefix, size_t prefix_len, const uint8_t* const* parts, const size_t* part_len, size_t nparts, uint64_t* out, size_t n)
{
    return hash_rows_call(ctx, zc::k_ris_from_sha512, prefix, prefix_len, parts, part_len, nparts, out, "out", 20, n);
}
int zc_proj_add(zc_ctx* c, const uint64_t* p, const uint64_t* q, uint64_t* o, size_t n) { return binop(c, zc::k_proj_add, p, q, o, n, 15); }
int zc_proj_double(zc_ctx* c, const uint64_t* p, uint64_t* o, size_t n) { return unop(c, zc::k_proj_double, p, o, n, 15); }
int zc_proj_to_extended(zc_ctx* ctx, const uint64_t* p, uint64_t* out, size_t n) { return batched(ctx, n, false, plain(zc::k_proj_to_extended), ROWS(p, 15), ROWS(out, 20)); }
// E-x rows: coset4 and the remaining ProjectivePoint operations
int zc_ed_coset4(zc_ctx* ctx, const uint64_t* p, uint64_t* out4, size_t n) { return batched(ctx, n, false, plain(zc::k_ed_coset4), ROWS(p, 20), ROWS(out4, 80)); }
int zc_proj_neg(zc_ctx* c, const uint64_t* p, uint64_t* o, size_t n) { return unop(c, zc::k_proj_neg, p, o, n, 15); }
int zc_proj_sub(zc_ctx* c, const uint64_t* p, const uint64_t* q, uint64_t* o, size_t n) { return binop(c, zc::k_proj_sub, p, q, o, n, 15); }
int zc_proj_eq(zc_ctx* ctx, const uint64_t* p, const uint64_t* q, uint8_t* eq, size_t n) { return batched(ctx, n, false, plain(zc::k_proj_eq), ROWS(p, 15), ROWS(q, 15), ROWS(eq, 1)); }
int zc_proj_is_valid(zc_ctx* ctx, const uint64_t* p, uint8_t* valid, size_t n) { return batched(ctx, n, false, plain(zc::k_proj_is_valid), ROWS(p, 15), ROWS(valid, 1)); }
int zc_proj_scalar_mul(zc_ctx* ctx, const uint64_t* p, const uint64_t* k, uint64_t* out, size_t n)
{
    return batched(ctx, n, false, plain(zc::k_proj_scalar_mul), ROWS(p, 15), ROWS(k, 5), ROWS(out, 15));
}

// ---- fixed-base multiplication of the basepoint
// A table the slot builds on first use and keeps: allocated once, filled by `builder` (one workgroup of `block` lanes) on D.s().
// A builder whose launch is refused leaves no table behind.
static int lazy_table(DevState& D, DevBuf& buf, size_t bytes, void (*builder)(zc::u32*), unsigned block, const zc::u32** table)
{
    if (!buf) {
        if (int rc = buf.grow(bytes)) return rc;
        hipLaunchKernelGGL(builder, dim3(1), dim3(block), 0, D.s(), buf.as<zc::u32>());
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            (void)buf.reset();
            return fail(ZC_ERR_HIP, "device table build", e);
        }
    }
    *table = buf.as<const zc::u32>();
    return ZC_OK;
}
static int base_table(DevState& D, const zc::u32** table)
{
    return lazy_table(D, D.base_table, (size_t)zc::ZC_BASE_WINDOWS * zc::ZC_BASE_ENTRIES * 128, zc::k_base_table_build, zc::ZC_BASE_ENTRIES, table);
}
static int odd_table(DevState& D, const zc::u32** table)
{
    return lazy_table(D, D.odd_table, (size_t)zc::ZC_ODD_ENTRIES * 128, zc::k_odd_table_build, 128, table);
}
int zc_ed_mul_base(zc_ctx* ctx, const uint64_t* k, uint64_t* out, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* dk, u64* dout) -> int {
        const zc::u32* t = nullptr;
        if (int rc = base_table(D, &t)) return rc;
        hipLaunchKernelGGL(zc::k_ed_mul_base, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dk, dout, t, cnt);
        return ZC_OK;
    }, ROWS(k, 5), ROWS(out, 20));
}
int zc_ris_mul_base_compress(zc_ctx* ctx, const uint64_t* k, uint8_t* out32, size_t n)
{
    return batched(ctx, n, false, [](DevState& D, size_t cnt, const u64* dk, uint8_t* dout) -> int {
        const zc::u32* t = nullptr;
        if (int rc = base_table(D, &t)) return rc;
        hipLaunchKernelGGL(zc::k_ris_mul_base_compress, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dk, dout, t, cnt);
        return ZC_OK;
    }, ROWS(k, 5), ROWS(out32, 32));
}
// out32[i] = compress(base_scalars[i] * B + sum_j scalars[i][j] * decompress(in32[i][j])): zc_ed_lincomb's windowed core between
// the two codecs, the basepoint term from the comb table (zc_kernels.hip.h: k_ris_lincomb)
int zc_ris_lincomb(zc_ctx* ctx, const uint8_t* in32, const uint64_t* scalars, size_t terms, const uint64_t* base_scalars, uint8_t* out32,
                   uint8_t* ok, size_t n)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    const size_t slots_used = terms + (base_scalars ? 1 : 0);             // the base term takes one of the scalar slots
    if (terms < 1 || terms > ZC_LINCOMB_MAX_TERMS || slots_used > ZC_LINCOMB_MAX_TERMS)
        return fail(ZC_ERR_BAD_ARG, "zc_ris_lincomb: terms must be at least 1, terms + (base_scalars != NULL) at most ZC_LINCOMB_MAX_TERMS");
    if (n >= ((size_t)1 << 31) / terms + (((size_t)1 << 31) % terms != 0)) return fail(ZC_ERR_BAD_ARG, "zc_ris_lincomb: n * terms must stay below 2^31");
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const uint8_t* din, const u64* dk, const u64* dbase, uint8_t* dout, uint8_t* dok) -> int {
        const zc::u32* comb = nullptr;
        if (dbase)
            if (int rc = base_table(D, &comb)) return rc;
        const zc::LincombLaunch ll = zc::lincomb_launch(slots_used);
        const zc::u32 units = (zc::u32)zc::ring_units_per_xcd(terms);
        return fast_ring(D, cnt, [&](zc::u32* table, zc::u32* ring, zc::u32 slots, size_t off, size_t c) {
            hipLaunchKernelGGL(zc::k_ris_lincomb, dim3((unsigned)((c + ll.block - 1) / ll.block)), dim3(ll.block), ll.lds_bytes, D.s(),
                               din + 32 * terms * off, dk + 5 * terms * off, (zc::u32)terms, dbase ? dbase + 5 * off : nullptr, dout + 32 * off,
                               dok ? dok + off : nullptr, comb, table, ring, slots, units, (zc::u32)terms, (zc::u32)c);
        }, terms);
    }, ROWS(in32, 32 * terms), ROWS(scalars, 5 * terms), OPT_ROWS(base_scalars, 5), ROWS(out32, 32), OPT_ROWS(ok, 1));
}

// window_naf_mul (src/edwards.rs:155-171) with its table indexed correctly: see k_ed_mul_base_wnaf
int zc_ed_mul_base_wnaf(zc_ctx* ctx, const uint64_t* k, unsigned width, uint64_t* out, size_t n)
{
    if (width < 2 || width > 7) return fail(ZC_ERR_BAD_ARG, "zc_ed_mul_base_wnaf: window width 2..7 (compute_window_NAF's digits are i8)");
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* dk, u64* dout) -> int {
        const zc::u32* t = nullptr;
        if (int rc = odd_table(D, &t)) return rc;
        hipLaunchKernelGGL(zc::k_ed_mul_base_wnaf, dim3(grid_for(cnt)), dim3(zc::ZC_BLOCK), 0, D.s(), dk, (zc::u32)width, dout, t, cnt);
        return ZC_OK;
    }, ROWS(k, 5), ROWS(out, 20));
}

// ---- generator sets (zerocaf_hip_ext_gens.h): the basepoint's comb over caller-supplied points (zc_gens.hip.h)
// The tables of one device slot: the points uploaded, checked and normalised by the builder itself, which reports a generator
// that is no curve point in `bad`.  Everything enqueued is through before the staging block goes.
static int gens_build_on(DevState& D, const u64* host_points, size_t count, DevBuf& tables, int* first_bad)
{
    if (int rc = ring_check(D)) return rc;
    HIP_TRY(hipSetDevice(D.device));
    if (int rc = tables.alloc(count * zc::GENS_TABLE_WORDS * sizeof(zc::u32), "zc_gens_create: hipMalloc(tables)")) return rc;
    DevBuf stage;                                           // the points, then one flag per generator
    if (int rc = stage.alloc(count * 160 + count * sizeof(zc::u32), "zc_gens_create: hipMalloc(points)")) return rc;
    u64* const dpts = stage.as<u64>();
    zc::u32* const dbad = reinterpret_cast<zc::u32*>(dpts + 20 * count);
    zc::u32 bad[ZC_GENS_MAX] = {};
    if (int rc = enqueue_and_drain(D, "zc_gens_create: table build", [&](const char* what) -> int {
            HIP_TRY_AS(hipMemcpyAsync(dpts, host_points, count * 160, hipMemcpyHostToDevice, D.s()), what);
            HIP_TRY_AS(hipMemsetAsync(dbad, 0, count * sizeof(zc::u32), D.s()), what);
            hipLaunchKernelGGL(zc::k_gens_table_build, dim3((unsigned)count), dim3(zc::ZC_BASE_ENTRIES), 0, D.s(), (const u64*)dpts, tables.as<zc::u32>(), dbad);
            HIP_TRY_AS(hipGetLastError(), what);
            HIP_TRY_AS(hipMemcpyAsync(bad, dbad, count * sizeof(zc::u32), hipMemcpyDeviceToHost, D.s()), what);
            return ZC_OK;
        }))
        return rc;
    for (size_t j = count; j-- > 0;)
        if (bad[j]) *first_bad = (int)j;
    return ZC_OK;
}
int zc_gens_create(zc_ctx* ctx, const uint64_t* points, size_t count, uint64_t* id_out)
{
    REQUIRE(points);
    REQUIRE(id_out);
    if (count < 1 || count > ZC_GENS_MAX) return fail(ZC_ERR_BAD_ARG, "zc_gens_create: count must be 1 .. ZC_GENS_MAX");
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    u64 host[20 * ZC_GENS_MAX];                             // device-resident points come down once and go up to every slot
    if (int rc = fetch_once(ctx, "zc_gens_create: ", points, host, count * 160)) return rc;
    GenSet g{count, std::vector<DevBuf>(ctx->devs.size())};
    int first_bad = -1;
    int rc = ZC_OK;
    for (size_t di = 0; di < ctx->devs.size() && !rc && first_bad < 0; di++) rc = gens_build_on(ctx->devs[di], host, count, g.mem[di], &first_bad);
    (void)hipSetDevice(ctx->devs[0].device);
    if (rc) return rc;
    if (first_bad >= 0) return failf(ZC_ERR_BAD_ARG, "zc_gens_create: generator %d is not a point of the curve", first_bad);
    *id_out = ctx->gens.add(std::move(g));
    return ZC_OK;
}
int zc_gens_destroy(zc_ctx* ctx, uint64_t id) { return table_destroy(ctx, &zc_ctx::gens, id, NO_GENS); }
int zc_ed_mul_gens(zc_ctx* ctx, uint64_t id, const uint64_t* scalars, uint64_t* out, size_t n)
{
    REQUIRE(scalars);
    REQUIRE(out);
    return mul_gens(ctx, id, scalars, out, 20, n, "zc_ed_mul_gens", zc::k_ed_mul_gens);
}
int zc_ris_mul_gens_compress(zc_ctx* ctx, uint64_t id, const uint64_t* scalars, uint8_t* out32, size_t n)
{
    REQUIRE(scalars);
    REQUIRE(out32);
    return mul_gens(ctx, id, scalars, out32, 32, n, "zc_ris_mul_gens_compress", zc::k_ris_mul_gens_compress);
}

// ---- point sums (zerocaf_hip_ext_sum_rows.h): out[i] = P_i0 + P_i1 + ... in the order zc_sum_plan.h fixes for `terms` (kernels:
// zc_sum.hip.h; launches: sum_rows_launch).  The checks behind the pointers, in the header's order.
static int sum_rows_args(zc_ctx* ctx, size_t n, size_t terms, const char* who)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (zc::sum_too_large(n, terms)) return failf(ZC_ERR_BAD_ARG, "%s: n * terms must stay below 2^31", who);
    return ZC_OK;
}
int zc_ed_sum_rows(zc_ctx* ctx, const uint64_t* points, size_t terms, uint64_t* out, size_t n)
{
    REQUIRE(points);
    REQUIRE(out);
    if (int rc = sum_rows_args(ctx, n, terms, "zc_ed_sum_rows")) return rc;
    if (terms == 0)                                         // nothing of `points` is read: identity rows
        return batched(ctx, n, false, [&](DevState& D, size_t cnt, u64* dout) -> int {
            return sum_rows_launch(D, cnt, 0, zc::k_ed_rowsum, zc::k_ed_rowsum_part, zc::k_ed_rowsum_finish, (const u64*)nullptr, dout);
        }, ROWS(out, 20));
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* dp, u64* dout) -> int {
        return sum_rows_launch(D, cnt, terms, zc::k_ed_rowsum, zc::k_ed_rowsum_part, zc::k_ed_rowsum_finish, dp, dout);
    }, ROWS(points, 20 * terms), ROWS(out, 20));
}
int zc_ris_sum_rows(zc_ctx* ctx, const uint8_t* in32, size_t terms, uint8_t* out32, uint8_t* ok, size_t n)
{
    REQUIRE(in32);
    REQUIRE(out32);
    if (int rc = sum_rows_args(ctx, n, terms, "zc_ris_sum_rows")) return rc;
    if (terms == 0)
        return batched(ctx, n, false, [&](DevState& D, size_t cnt, uint8_t* dout, uint8_t* dok) -> int {
            return sum_rows_launch(D, cnt, 0, zc::k_ris_rowsum, zc::k_ris_rowsum_part, zc::k_ris_rowsum_finish, (const uint8_t*)nullptr, dout, dok);
        }, ROWS(out32, 32), OPT_ROWS(ok, 1));
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const uint8_t* din, uint8_t* dout, uint8_t* dok) -> int {
        return sum_rows_launch(D, cnt, terms, zc::k_ris_rowsum, zc::k_ris_rowsum_part, zc::k_ris_rowsum_finish, din, dout, dok);
    }, ROWS(in32, 32 * terms), ROWS(out32, 32), OPT_ROWS(ok, 1));
}

// ---- bounded discrete logs (zerocaf_hip_dlog.h): baby steps from a table, giant steps per row (kernels: zc_dlog.hip.h; sizes,
// slices and the slot array: zc_dlog_plan.h)
// Slot 0's share of zc_dlog_create: the setup block and the records, computed there and brought to the host.
static int dlog_compute_on(DevState& D, const u64* host_point, DlogTable& tb, std::vector<u64>& records)
{
    if (int rc = ring_check(D)) return rc;
    HIP_TRY(hipSetDevice(D.device));
    DevBuf stage;                                           // the point, then the setup block
    if (int rc = stage.alloc(160 + zc::DLOG_SETUP_WORDS * sizeof(zc::u32), "zc_dlog_create: hipMalloc(setup)")) return rc;
    u64* const dpoint = stage.as<u64>();
    zc::u32* const dsetup = reinterpret_cast<zc::u32*>(dpoint + 20);
    tb.setup.assign(zc::DLOG_SETUP_WORDS, 0);
    if (int rc = enqueue_and_drain(D, "zc_dlog_create: setup", [&](const char* what) -> int {
            HIP_TRY_AS(hipMemcpyAsync(dpoint, host_point, 160, hipMemcpyHostToDevice, D.s()), what);
            HIP_TRY_AS(hipMemsetAsync(dsetup, 0, zc::DLOG_SETUP_WORDS * sizeof(zc::u32), D.s()), what);
            hipLaunchKernelGGL(zc::k_dlog_setup, dim3(1), dim3(zc::DLOG_BLOCK), 0, D.s(), (const u64*)dpoint, dsetup, (zc::u32)tb.t, (zc::u32)tb.flags);
            HIP_TRY_AS(hipGetLastError(), what);
            HIP_TRY_AS(hipMemcpyAsync(tb.setup.data(), dsetup, zc::DLOG_SETUP_WORDS * sizeof(zc::u32), hipMemcpyDeviceToHost, D.s()), what);
            return ZC_OK;
        }))
        return rc;
    if (tb.setup[0] == zc::DLOG_SETUP_NOT_A_POINT) return fail(ZC_ERR_BAD_ARG, "zc_dlog_create: not a point of the curve");
    if (tb.setup[0] != zc::DLOG_SETUP_OK) return fail(ZC_ERR_BAD_ARG, "zc_dlog_create: generator lies in E[8]");
    if (int rc = tb.mem[0].alloc(zc::dlog_table_bytes(tb.t), "zc_dlog_create: hipMalloc(table)")) return rc;
    records.resize(4 * zc::dlog_records(tb.t));
    const size_t lanes = zc::dlog_build_lanes(tb.t);
    return enqueue_and_drain(D, "zc_dlog_create: records", [&](const char* what) -> int {
        hipLaunchKernelGGL(zc::k_dlog_records, dim3((unsigned)((lanes + zc::DLOG_BLOCK - 1) / zc::DLOG_BLOCK)), dim3(zc::DLOG_BLOCK), 0, D.s(), (const zc::u32*)dsetup,
                           tb.mem[0].as<u64>(), (zc::u32)tb.t);
        HIP_TRY_AS(hipGetLastError(), what);
        HIP_TRY_AS(hipMemcpyAsync(records.data(), tb.mem[0].as<u64>(), zc::dlog_record_bytes(tb.t), hipMemcpyDeviceToHost, D.s()), what);
        return ZC_OK;
    });
}
int zc_dlog_create(zc_ctx* ctx, const uint64_t* point, unsigned table_bits, unsigned flags, uint64_t* id_out)
{
    REQUIRE(point);
    REQUIRE(id_out);
    if (!zc::dlog_bits_ok(table_bits)) return fail(ZC_ERR_BAD_ARG, "zc_dlog_create: table_bits must be ZC_DLOG_MIN_BITS .. ZC_DLOG_MAX_BITS");
    if (flags & ~ZC_DLOG_COSET4) return fail(ZC_ERR_BAD_ARG, "zc_dlog_create: unknown flag bits");
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    u64 host[20];                                           // a device-resident point comes down once
    if (int rc = fetch_once(ctx, "zc_dlog_create: ", point, host, 160)) return rc;
    DlogTable tb{table_bits, flags, {}, std::vector<DevBuf>(ctx->devs.size())};
    std::vector<u64> records, slots;
    int rc = dlog_compute_on(ctx->devs[0], host, tb, records);
    if (!rc) {
        slots.resize(zc::dlog_slots(tb.t));
        if (zc::dlog_build_slots(slots.data(), tb.t, records.data()) >= 0) rc = fail(ZC_ERR_BAD_ARG, "zc_dlog_create: two table entries coincide");
    }
    // the slots behind the records on every device slot; the records too where they were not computed
    for (size_t di = 0; di < ctx->devs.size() && !rc; di++) {
        DevState& D = ctx->devs[di];
        DevBuf& mem = tb.mem[di];
        if (di && (rc = ring_check(D))) break;              // slot 0: dlog_compute_on has asked
        rc = enqueue_and_drain(D, "zc_dlog_create: table upload", [&](const char* what) -> int {
            HIP_TRY_AS(hipSetDevice(D.device), what);
            if (di) {
                if (int arc = mem.alloc(zc::dlog_table_bytes(tb.t), "zc_dlog_create: hipMalloc(table)")) return arc;
                HIP_TRY_AS(hipMemcpyAsync(mem.as<u64>(), records.data(), zc::dlog_record_bytes(tb.t), hipMemcpyHostToDevice, D.s()), what);
            }
            HIP_TRY_AS(hipMemcpyAsync(mem.as<u64>() + 4 * zc::dlog_records(tb.t), slots.data(), zc::dlog_slot_bytes(tb.t), hipMemcpyHostToDevice, D.s()), what);
            return ZC_OK;
        });
    }
    (void)hipSetDevice(ctx->devs[0].device);
    if (rc) return rc;
    *id_out = ctx->dlogs.add(std::move(tb));
    return ZC_OK;
}
int zc_dlog_destroy(zc_ctx* ctx, uint64_t id) { return table_destroy(ctx, &zc_ctx::dlogs, id, NO_DLOG); }
// The checks of the two row calls behind their pointers, in the header's order.
static int dlog_row_args(zc_ctx* ctx, uint64_t id, uint64_t bound, size_t n, bool wire, const char* who)
{
    unsigned t = 0, flags = 0;
    if (int rc = table_facts(ctx, &zc_ctx::dlogs, id, NO_DLOG, [&](const DlogTable& tb) { t = tb.t, flags = tb.flags; })) return rc;
    if (wire && !(flags & ZC_DLOG_COSET4)) return fail(ZC_ERR_BAD_ARG, "zc_ris_dlog needs a ZC_DLOG_COSET4 table");
    if (!zc::dlog_bound_ok(bound, t)) return failf(ZC_ERR_BAD_ARG, "%s: bound must be 1 .. 2^table_bits * ZC_DLOG_MAX_STEPS", who);
    if (n >= ((size_t)1 << 31)) return failf(ZC_ERR_BAD_ARG, "%s: n must stay below 2^31", who);
    return ZC_OK;
}
int zc_ed_dlog(zc_ctx* ctx, uint64_t id, const uint64_t* p, uint64_t bound, uint64_t* m_out, uint8_t* found, uint8_t* ok, size_t n)
{
    REQUIRE(p);
    REQUIRE(m_out);
    REQUIRE(found);
    if (int rc = dlog_row_args(ctx, id, bound, n, false, "zc_ed_dlog")) return rc;
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const u64* dp, u64* dm, uint8_t* df, uint8_t* dok) -> int {
        return dlog_launches_on(ctx, id, D, zc::k_ed_dlog, dp, bound, dm, df, dok, cnt);
    }, ROWS(p, 20), ROWS(m_out, 1), ROWS(found, 1), OPT_ROWS(ok, 1));
}
int zc_ris_dlog(zc_ctx* ctx, uint64_t id, const uint8_t* in32, uint64_t bound, uint64_t* m_out, uint8_t* found, uint8_t* ok, size_t n)
{
    REQUIRE(in32);
    REQUIRE(m_out);
    REQUIRE(found);
    if (int rc = dlog_row_args(ctx, id, bound, n, true, "zc_ris_dlog")) return rc;
    return batched(ctx, n, true, [&](DevState& D, size_t cnt, const uint8_t* din, u64* dm, uint8_t* df, uint8_t* dok) -> int {
        return dlog_launches_on(ctx, id, D, zc::k_ris_dlog, din, bound, dm, df, dok, cnt);
    }, ROWS(in32, 32), ROWS(m_out, 1), ROWS(found, 1), OPT_ROWS(ok, 1));
}

// ---- scalar vector ops (zerocaf_hip_scvec.h): row sums, inner products and power rows mod L (kernels: zc_scvec.hip.h; the cut of
// a row, the forms and the grids: zc_scvec_plan.h).  The checks behind the pointers, in the header's order.
static int scvec_args(zc_ctx* ctx, size_t n, size_t terms, const char* who)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (zc::scv_too_large(n, terms)) return failf(ZC_ERR_BAD_ARG, "%s: n * terms must stay below 2^31", who);
    return ZC_OK;
}
// The launches of `cnt` rows of a sum (b null) or a dot product on slot D: one kernel (the block form, or a row per workgroup), or
// -- more slices than a workgroup has lanes -- the first kernel into the slot's `scvec` workspace and the one that finishes the rows, both on the slot's stream (a later
// call's kernels come behind them; a workspace that has to grow is freed first, which waits for the device).
static int scvec_rows_launch(DevState& D, size_t cnt, size_t terms, const u64* a, const u64* b, bool shared_b, u64* out)
{
    const zc::ScvPlan p = zc::scv_plan(cnt, terms);
    if (p.grid1 >= ((size_t)1 << 31)) return fail(ZC_ERR_BAD_ARG, "more rows than one launch holds");       // rows without terms only: n * terms < 2^31 bounds every other grid
    const zc::u32 t = (zc::u32)terms, parts = (zc::u32)p.parts, sh = shared_b ? 1u : 0u;
    if (p.form == zc::SCV_FORM_BLOCK) {
        if (b) hipLaunchKernelGGL(zc::k_sc_rowdot, dim3((unsigned)p.grid1), dim3(zc::SCV_BLOCK), 0, D.s(), a, b, sh, t, parts, out, cnt);
        else hipLaunchKernelGGL(zc::k_sc_rowsum, dim3((unsigned)p.grid1), dim3(zc::SCV_BLOCK), 0, D.s(), a, t, parts, out, cnt);
        return ZC_OK;
    }
    if (p.form == zc::SCV_FORM_ROW) {
        if (b) hipLaunchKernelGGL(zc::k_sc_rowdot_long, dim3((unsigned)p.grid1), dim3(zc::SCV_BLOCK), 0, D.s(), a, b, sh, t, parts, out);
        else hipLaunchKernelGGL(zc::k_sc_rowsum_long, dim3((unsigned)p.grid1), dim3(zc::SCV_BLOCK), 0, D.s(), a, t, parts, out);
        return ZC_OK;
    }
    if (int rc = D.scvec.grow(p.workspace_bytes)) return rc;
    zc::u32* const ws = D.scvec.as<zc::u32>();
    if (b) hipLaunchKernelGGL(zc::k_sc_rowdot_part, dim3((unsigned)p.grid1), dim3(zc::SCV_BLOCK), 0, D.s(), a, b, sh, t, parts, ws);
    else hipLaunchKernelGGL(zc::k_sc_rowsum_part, dim3((unsigned)p.grid1), dim3(zc::SCV_BLOCK), 0, D.s(), a, t, parts, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(zc::k_sc_rows_finish, dim3((unsigned)p.grid2), dim3(zc::SCV_BLOCK), 0, D.s(), (const zc::u32*)ws, (zc::u32)p.blocks_per_row, out, cnt);
    return ZC_OK;
}
// Rows without terms are zero: nothing of the inputs is read.
static int scvec_zero_rows(zc_ctx* ctx, uint64_t* out, size_t n)
{
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, u64* dout) -> int { return scvec_rows_launch(D, cnt, 0, nullptr, nullptr, false, dout); }, ROWS(out, 5));
}
int zc_sc_sum_rows(zc_ctx* ctx, const uint64_t* a, size_t terms, uint64_t* out, size_t n)
{
    REQUIRE(a);
    REQUIRE(out);
    if (int rc = scvec_args(ctx, n, terms, "zc_sc_sum_rows")) return rc;
    if (terms == 0) return scvec_zero_rows(ctx, out, n);
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, u64* dout) -> int {
        return scvec_rows_launch(D, cnt, terms, da, nullptr, false, dout);
    }, ROWS(a, 5 * terms), ROWS(out, 5));
}
int zc_sc_dot_rows(zc_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t terms, unsigned flags, uint64_t* out, size_t n)
{
    REQUIRE(a);
    REQUIRE(b);
    REQUIRE(out);
    if (flags & ~ZC_SC_DOT_SHARED_B) return fail(ZC_ERR_BAD_ARG, "zc_sc_dot_rows: unknown flag bits");
    if (int rc = scvec_args(ctx, n, terms, "zc_sc_dot_rows")) return rc;
    if (n == 0) return ZC_OK;
    if (terms == 0) return scvec_zero_rows(ctx, out, n);
    if (!(flags & ZC_SC_DOT_SHARED_B))
        return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, const u64* db, u64* dout) -> int {
            return scvec_rows_launch(D, cnt, terms, da, db, false, dout);
        }, ROWS(a, 5 * terms), ROWS(b, 5 * terms), ROWS(out, 5));
    // one row of b for every row: it is no buffer of rows, so its place is asked here.  On the device it is used where it lies;
    // from host memory it goes to each device slot once, on the slot's stream in front of the slot's first kernel (the call holds
    // the context's lock and ends synchronised, so the copy in `scvec_b` has no other reader).
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, {a, b, out}, "", &owner)) return rc;
    std::vector<char> sent(ctx->devs.size(), 0);
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* da, u64* dout) -> int {
        const u64* db = b;
        if (!owner) {
            if (!sent[D.slot]) {
                if (int rc = D.scvec_b.grow(40 * terms)) return rc;
                HIP_TRY(hipMemcpyAsync(D.scvec_b.as<void>(), b, 40 * terms, hipMemcpyHostToDevice, D.s()));
                sent[D.slot] = 1;
            }
            db = D.scvec_b.as<const u64>();
        }
        return scvec_rows_launch(D, cnt, terms, da, db, true, dout);
    }, ROWS(a, 5 * terms), ROWS(out, 5));
}
int zc_sc_powers(zc_ctx* ctx, const uint64_t* x, size_t terms, uint64_t* out, size_t n)
{
    REQUIRE(x);
    REQUIRE(out);
    if (int rc = scvec_args(ctx, n, terms, "zc_sc_powers")) return rc;
    if (terms == 0) return ZC_OK;                           // nothing to write
    return batched(ctx, n, false, [&](DevState& D, size_t cnt, const u64* dx, u64* dout) -> int {
        const zc::ScvPowPlan p = zc::scv_pow_plan(cnt, terms);
        hipLaunchKernelGGL(zc::k_sc_powers, dim3((unsigned)p.grid), dim3(zc::SCV_BLOCK), 0, D.s(), dx, (zc::u32)terms, (zc::u32)p.group, dout, cnt);
        return ZC_OK;
    }, ROWS(x, 5), ROWS(out, 5 * terms));
}

// ---- MSM: sum_i k_i * P_i (not in the reference; specified as the reference's own
// sum of `&P_i * &k_i`, src/edwards.rs:547-561 + :465-489).  Per GPU: bucket method (zc_msm.hip.h)
// for shards of >= MSM_BUCKET_MIN_N pairs, otherwise batched scalar-mul + pairwise folds.
// The exchange step lives here: per-device partial sums are gathered INTO DEVICE MEMORY
// (hipMemcpyPeerAsync inside one process, ncclAllGather between processes) and folded in
// device / rank order by ONE kernel (k_ed_fold_ordered), so every rank ends with identical limbs.

// partial sums of all device slots -> slot 0's `part` buffer, folded there; result at part[nparts]
static int gather_and_fold(zc_ctx* ctx, const std::vector<DevState*>& used, const std::vector<const u64*>& partial_ptr, const u64** result)
{
    DevState* d0 = used[0];
    const size_t np = used.size();
    if (np == 1) {
        *result = partial_ptr[0];
        return ZC_OK;
    }
    HIP_TRY(hipSetDevice(d0->device));
    if (int rc = d0->part.grow((np + 1) * 160)) return rc;
    u64* part = d0->part.as<u64>();
    for (size_t ui = 0; ui < np; ui++) {
        DevState* ds = used[ui];
        HIP_TRY(hipSetDevice(ds->device));
        if (ds->device == d0->device) HIP_TRY(hipMemcpyAsync(part + 20 * ui, partial_ptr[ui], 160, hipMemcpyDeviceToDevice, ds->s()));
        else HIP_TRY(hipMemcpyPeerAsync(part + 20 * ui, d0->device, partial_ptr[ui], ds->device, 160, ds->s()));
        if (ds != d0) {
            HIP_TRY(hipEventRecord(ds->ev_order, ds->s()));
            HIP_TRY(hipStreamWaitEvent(d0->s(), ds->ev_order, 0));
        }
    }
    HIP_TRY(hipSetDevice(d0->device));
    hipLaunchKernelGGL(zc::k_ed_fold_ordered, dim3(1), dim3(64), 0, d0->s(), (const u64*)part, np, (const u64*)nullptr, part + 20 * np);
    HIP_TRY(hipGetLastError());
    *result = part + 20 * np;
    return ZC_OK;
}

// local part of an MSM over every device slot of the context (host inputs: contiguous shards, one
// worker thread per slot; device inputs: the owning slot); *result in device memory of *owner
static int msm_local(zc_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n, DevState** owner, const u64** result)
{
    DevState* ds = nullptr;
    if (int rc = owner_of(ctx, {points, scalars}, "", &ds)) return rc;
    std::vector<DevState*> used;
    std::vector<const u64*> partial_ptr;
    if (ds) {
        const u64* part = nullptr;
        int rc = msm_shard(*ds, points, scalars, n, true, &part);
        if (rc) return rc;
        *owner = ds;
        *result = part;
        return ZC_OK;
    }
    const size_t ndev = ctx->devs.size();
    const size_t per = (n + ndev - 1) / ndev;
    size_t nshards = 0;
    while (nshards < ndev && nshards * per < n) nshards++;
    std::vector<int> rcs(nshards, ZC_OK);
    std::vector<std::string> errs(nshards);
    partial_ptr.assign(nshards, nullptr);
    auto job = [&](size_t di) {
        const size_t lo = di * per, hi = std::min(n, lo + per);
        rcs[di] = msm_shard(ctx->devs[di], points + 20 * lo, scalars + 5 * lo, hi - lo, false, &partial_ptr[di]);
        if (rcs[di]) errs[di] = g_last_error;
    };
    std::vector<std::thread> workers;                       // pageable uploads block their thread: one per device
    for (size_t di = 1; di < nshards; di++) workers.emplace_back(job, di);
    job(0);
    for (auto& t : workers) t.join();
    for (size_t di = 0; di < nshards; di++) {
        if (rcs[di]) {
            g_last_error = errs[di];
            return rcs[di];
        }
        used.push_back(&ctx->devs[di]);
    }
    *owner = used[0];
    return gather_and_fold(ctx, used, partial_ptr, result);
}

int zc_msm(zc_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n, uint64_t* out_point)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(points); REQUIRE(scalars); REQUIRE(out_point);
    if (n == 0) {
        memcpy(out_point, IDENT_POINT, sizeof IDENT_POINT);
        return ZC_OK;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState* owner = nullptr;
    const u64* res = nullptr;
    int rc = msm_local(ctx, points, scalars, n, &owner, &res);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(owner->device));
    HIP_TRY(hipMemcpyAsync(out_point, res, 160, hipMemcpyDeviceToHost, owner->s()));
    HIP_TRY(hipStreamSynchronize(owner->s()));
    return ZC_OK;
}

#ifdef ZC_TEST_HOOKS
// Test hook, compiled only into libzerocaf_hip_test.so (-DZC_TEST_HOOKS), NOT part of the ABI (not in include/zerocaf_hip.h,
// not mirrored): the MSM's digit + sort stage alone.
// `scalars` (n x 5 u64) and `out_pairs` (n * ceil(261 / c) pairs of u32: bucket key, point index | sign << 31)
// are DEVICE buffers of ctx's device slot 0; synchronises before returning.
int zc_test_msm_sort(zc_ctx* ctx, const uint64_t* scalars, size_t n, int c, uint32_t* out_pairs)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(scalars); REQUIRE(out_pairs);
    if (c < zc::MSM_MIN_C || c > zc::MSM_MAX_C || n == 0) return fail(ZC_ERR_BAD_ARG, "zc_test_msm_sort: bad window width / empty batch");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState& D = ctx->devs[0];
    HIP_TRY(hipSetDevice(D.device));
    const int W = zc::msm_windows(c);
    if (zc::msm_index_limit(0, zc::msm_sat_mul(n, (size_t)W), 0)) return fail(ZC_ERR_BAD_ARG, "zc_test_msm_sort: too many pairs");
    const zc::MsmKnobs& knobs = D.tune.msm;
    const MsmBucketPlan bp = msm_bucket_plan(n, (size_t)W, c, false, knobs);
    const MsmSortPlan& plan = bp.sort;
    MsmWorkspace ws;
    if (int rc = msm_workspace(D, bp, 0, 0, &ws, true)) return rc;
    hipLaunchKernelGGL(zc::k_msm_digits, dim3(grid_for(n)), dim3(zc::ZC_BLOCK), 0, D.s(), (const u64*)scalars, ws.digits, n, c, W);
    // ZC_MSM_GROUPS that adds up to the windows: every group sorted on its own, top group first (the per-group sort that was
    // measured against msm_on_device's one sort)
    int gsum = 0;
    for (int g = 0; g < knobs.ngroups; g++) gsum += knobs.groups[g];
    const bool split = knobs.ngroups >= 2 && gsum == W;
    for (int g = 0, top = W; top > 0; g++) {
        const int nw = split ? knobs.groups[g] : W;
        top -= nw;
        if (int rc = msm_sort(D, D.s(), plan, top, nw, ws.digits, ws.pairs_a, ws.pairs_b, ws.sort_table, plan.table_words, ws.sort_sums)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(out_pairs, ws.pairs_a, bp.m * sizeof(uint2), hipMemcpyDeviceToDevice, D.s()));
    HIP_TRY(hipStreamSynchronize(D.s()));
    HIP_TRY(hipGetLastError());
    return ZC_OK;
}
// Test hook: the w-NAF's odd-multiples table as the device built it, as 125 points in DEVICE memory of slot 0.
int zc_test_odd_table(zc_ctx* ctx, uint64_t* out_dev_points)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(out_dev_points);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState& D = ctx->devs[0];
    HIP_TRY(hipSetDevice(D.device));
    const zc::u32* t = nullptr;
    if (int rc = odd_table(D, &t)) return rc;
    hipLaunchKernelGGL(zc::k_test_odd_table_dump, dim3(1), dim3(128), 0, D.s(), t, (u64*)out_dev_points);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(D.s()));
    return ZC_OK;
}
// Test hook: how many launches of this context took each kernel form so far (all device slots), counted where the answer of
// zc_launch_plan.h is consumed: counts[f] for the first min(n, LAUNCH_FORMS) enumerators f of zc::LaunchForm.  Lets a test assert
// that the form it names -- not another one -- produced the output it compared.
int zc_test_launch_forms(zc_ctx* ctx, uint64_t* counts, int n)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(counts);
    std::lock_guard<std::mutex> lock(ctx->mu);
    for (int f = 0; f < n && f < zc::LAUNCH_FORMS; f++) {
        counts[f] = 0;
        for (auto& d : ctx->devs) counts[f] += d.forms[f];
    }
    return ZC_OK;
}
// The same for the LDS-staged form of the element-wise / point kernels alone.
long long zc_test_staged_launches(zc_ctx* ctx)
{
    uint64_t counts[zc::FORM_STAGED + 1];
    return zc_test_launch_forms(ctx, counts, zc::FORM_STAGED + 1) == ZC_OK ? (long long)counts[zc::FORM_STAGED] : -1;
}
#endif  // ZC_TEST_HOOKS

// What the bucket method would do for a shard of n pairs on this context (its knobs included) -- a query, no device
// work.  A measurement aid: a roofline record counts the useful multiplications from c, W and the addition formula.
// Writes min(nout, 17) entries (nout >= 8): [0] window bits c (0: below the bucket threshold, n scalar multiplications + folds),
// [1] windows W, [2] 1 = affine records / 7-multiplication additions, 0 = projective / 8, [3] PAYLOAD bytes of a gathered
// record (112 / 128), [4] run length of the bucket-sum kernel (window groups: the top group's), [5] buckets per reduction
// segment, [6] sort passes, [7] window groups G, [8] record STRIDE in bytes (what a gather touches: one 128-byte line),
// [9..12] windows per group (top group first), [13..16] run length per group.
static int msm_plan_report(zc_ctx* ctx, const char* who, size_t n, int points_aligned16, int32_t (&v)[17])
{
    const MsmPlan p = msm_plan(n, points_aligned16 != 0, ctx->devs[0].tune.msm);
    if (p.bad_groups) return failf(ZC_ERR_BAD_ARG, "%s: ZC_MSM_GROUPS does not add up to this shard's window count", who);
    const bool b = p.buckets;
    const int32_t w[17] = {p.c, p.W, p.affine ? 1 : 0, b ? (p.affine ? zc::MSM_AFF_WORDS * 4 : 128) : 0, b ? p.gT[0] : 0, p.seg, p.sort.passes, b ? p.G : 0, b ? p.rec_bytes : 0,
                           p.gw[0], p.gw[1], p.gw[2], p.gw[3], p.gT[0], p.gT[1], p.gT[2], p.gT[3]};
    memcpy(v, w, sizeof w);
    return ZC_OK;
}
int zc_msm_plan(zc_ctx* ctx, size_t n, int points_aligned16, int32_t* out, int nout)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(out);
    if (nout < 8) return fail(ZC_ERR_BAD_ARG, "zc_msm_plan: nout < 8");
    int32_t v[17];
    if (int rc = msm_plan_report(ctx, "zc_msm_plan", n, points_aligned16, v)) return rc;
    memcpy(out, v, sizeof(int32_t) * (size_t)std::min(nout, 17));
    return ZC_OK;
}

// ---- fixed-base MSM: tables of precomputed bases, batched over scalar vectors

int zc_msm_bases_create(zc_ctx* ctx, const uint64_t* points, size_t n, int window_bits, uint64_t* id_out)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(points); REQUIRE(id_out);
    int c = 0, W = 0;
    if (int rc = msm_fixed_check(n, window_bits, &c, &W, "zc_msm_bases_create")) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, {points}, "zc_msm_bases_create: ", &owner)) return rc;
    DevState& D = owner ? *owner : ctx->devs[0];
    if (int rc = ring_check(D)) return rc;
    HIP_TRY(hipSetDevice(D.device));
    MsmBases t{D.slot, n, c, W, std::vector<DevBuf>(ctx->devs.size())};
    DevBuf& recs = t.mem[t.slot];
    // window 0 = the points (copied: 16-byte aligned, plain), window j = 2^c times window j - 1, each normalised into its part of
    // the table; the two n-point buffers live for this call only.  Whatever was enqueued is through before the buffers go: the
    // two point arrays with this call, the table too when a step failed
    DevBuf pts[2];
    if (int rc = enqueue_and_drain(D, "zc_msm_bases_create: table build", [&](const char* what) -> int {
            if (int arc = recs.alloc(n * (size_t)W * ZC_MSM_REC_STRIDE, "zc_msm_bases_create: hipMalloc(table)")) return arc;
            for (DevBuf& b : pts)
                if (int arc = b.alloc(n * 160, "zc_msm_bases_create: hipMalloc(points)")) return arc;
            const hipError_t e = hipMemcpyAsync(pts[0].as<void>(), points, n * 160, owner ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, D.s());
            if (e != hipSuccess) return fail(ZC_ERR_HIP, "zc_msm_bases_create: copy of the points", e);
            const zc::u32 rec_words = ZC_MSM_REC_STRIDE / 4;
            for (int j = 0; j < W; j++) {
                if (j) hipLaunchKernelGGL(zc::k_msm_fixed_double, dim3(grid_for(n)), dim3(zc::ZC_BLOCK), 0, D.s(), pts[(j - 1) & 1].as<const u64>(), pts[j & 1].as<u64>(), n, c);
                msm_prepare_affine(D.s(), pts[j & 1].as<const u64>(), recs.as<zc::u32>() + (size_t)j * n * rec_words, n, D.tune, rec_words);
            }
            HIP_TRY_AS(hipGetLastError(), what);
            return ZC_OK;
        }))
        return rc;
    *id_out = ctx->bases.add(std::move(t));
    return ZC_OK;
}

int zc_msm_bases_destroy(zc_ctx* ctx, uint64_t id)
{
    return table_destroy(ctx, &zc_ctx::bases, id, "zc_msm_bases_destroy: no live table of this context has this id");
}

// out_points[b] = sum_i k[b][i] P_i: digits of every vector (one launch), ONE key sort over the batch's vectors as its windows,
// then the lower half of the bucket method (msm_reduce_windows) down to one sum per vector, copied to the host.
int zc_msm_fixed(zc_ctx* ctx, uint64_t id, const uint64_t* scalars, size_t batch, uint64_t* out_points)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    MsmBases* found = nullptr;
    if (int rc = table_find(ctx, &zc_ctx::bases, id, "zc_msm_fixed: no live table of this context has this id", &found)) return rc;
    if (batch == 0) return ZC_OK;
    REQUIRE(scalars); REQUIRE(out_points);
    const MsmBases& t = *found;
    const size_t n = t.n;
    const int c = t.c;
    const zc::MsmLimit limit = zc::msm_index_limit(0, zc::msm_sat_mul(batch, n * (size_t)t.W), zc::msm_sat_mul(batch, (size_t)1 << (c - 1)));
    if (limit == zc::MSM_LIMIT_PAIRS) return fail(ZC_ERR_BAD_ARG, "zc_msm_fixed: batch x n x W does not fit 32-bit pair indices");
    if (limit == zc::MSM_LIMIT_KEYS) return fail(ZC_ERR_BAD_ARG, "zc_msm_fixed: batch x 2^(c-1) buckets do not fit 32-bit bucket keys");
    DevState& D = ctx->devs[t.slot];
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, {scalars}, "zc_msm_fixed: ", &owner)) return rc;
    if (owner && owner->device != D.device) return fail(ZC_ERR_MIXED_MEM, "zc_msm_fixed: scalars on another device than the table");
    const u64* dK = scalars;
    if (int rc = msm_stage(D, owner != nullptr, nullptr, 0, &dK, batch * n)) return rc;
    const MsmBucketPlan fp = msm_fixed_plan(n, c, batch, D.tune.msm);
    MsmWorkspace ws;
    if (int rc = msm_workspace(D, fp, 0, 0, &ws)) return rc;
    hipLaunchKernelGGL(zc::k_msm_fixed_digits, dim3(grid_for(batch * n)), dim3(zc::ZC_BLOCK), 0, D.s(), dK, ws.digits, n, batch, c, t.W);
    HIP_TRY(hipMemsetAsync(ws.present, 0, fp.nb, D.s()));
    if (int rc = msm_sort(D, D.s(), fp.sort, 0, (int)batch, ws.digits, ws.pairs_a, ws.pairs_b, ws.sort_table, fp.sort.table_words, ws.sort_sums)) return rc;
    u64* sums = nullptr;
    if (int rc = msm_reduce_windows(D, msm_reduce_bufs(fp, ws, t.mem[t.slot].as<const zc::u32>()), msm_reduce_flat(fp, ws), &sums)) return rc;
    // the folds leave the batch's sums as canonical extended points, one per vector in order
    HIP_TRY(hipMemcpyAsync(out_points, sums, batch * 160, hipMemcpyDeviceToHost, D.s()));
    HIP_TRY(hipStreamSynchronize(D.s()));
    return ZC_OK;
}

// What a table of n bases would be (window_bits 0 = the library's choice) -- a query, no device work.  Writes min(nout, 8)
// entries (nout >= 8): [0] window bits c, [1] windows W, [2] record stride in bytes, [3] run length of the bucket-sum kernel
// and [4] buckets per reduction segment for one scalar vector, [5] sort passes, [6] table MiB (rounded up), [7] window groups (1).
int zc_msm_fixed_plan(zc_ctx* ctx, size_t n, int window_bits, int32_t* out, int nout)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(out);
    if (nout < 8) return fail(ZC_ERR_BAD_ARG, "zc_msm_fixed_plan: nout < 8");
    int c = 0, W = 0;
    if (int rc = msm_fixed_check(n, window_bits, &c, &W, "zc_msm_fixed_plan")) return rc;
    const MsmBucketPlan p = msm_fixed_plan(n, c, 1, ctx->devs[0].tune.msm);
    const size_t mib = (n * (size_t)W * ZC_MSM_REC_STRIDE + ((size_t)1 << 20) - 1) >> 20;
    const int32_t v[8] = {c, W, ZC_MSM_REC_STRIDE, p.T, p.seg, p.sort.passes, (int32_t)mib, 1};
    memcpy(out, v, sizeof v);
    return ZC_OK;
}

// ---- batched variable-base MSM: many independent sums, each over its own points

// out_points[b] = sum_i k[b][i] P[b][i]: one pipeline over the whole batch (msm_batch_on_device), or zc_msm's own path for one
// instance.  Inputs host (staged, device slot 0) or both on one device of the context; synchronous.
int zc_msm_batch(zc_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n, size_t batch, uint64_t* out_points)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (batch == 0) return ZC_OK;
    REQUIRE(points); REQUIRE(scalars); REQUIRE(out_points);
    if (n == 0) {
        for (size_t b = 0; b < batch; b++) memcpy(out_points + 20 * b, IDENT_POINT, sizeof IDENT_POINT);
        return ZC_OK;
    }
    if (int rc = msm_batch_check(n, batch, ctx->devs[0].tune, "zc_msm_batch")) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, {points, scalars}, "zc_msm_batch: ", &owner)) return rc;
    DevState& D = owner ? *owner : ctx->devs[0];
    const u64* res = nullptr;
    if (batch == 1) {
        if (int rc = msm_shard(D, points, scalars, n, owner != nullptr, &res)) return rc;
    } else {
        const u64 *dP = points, *dK = scalars;
        if (int rc = msm_stage(D, owner != nullptr, &dP, n * batch, &dK, n * batch)) return rc;
        if (int rc = msm_batch_on_device(D, dP, dK, n, batch, &res)) return rc;
    }
    HIP_TRY(hipSetDevice(D.device));
    HIP_TRY(hipMemcpyAsync(out_points, res, batch * 160, hipMemcpyDeviceToHost, D.s()));
    HIP_TRY(hipStreamSynchronize(D.s()));
    return ZC_OK;
}

// What zc_msm_batch would do for `batch` instances of n pairs -- a query, no device work.  Writes min(nout, 8) entries
// (nout >= 8): [0] regime (0 = scalar multiplications + folds, 1 = buckets), [1] window bits c, [2] windows W, [3] 1 = affine
// records, [4] run length of the bucket-sum kernel, [5] buckets per reduction segment, [6] sort passes, [7] record stride in
// bytes.  One instance reports zc_msm's plan (the call takes zc_msm's path).  Fails where zc_msm_batch fails on its limits.
int zc_msm_batch_plan(zc_ctx* ctx, size_t n, size_t batch, int points_aligned16, int32_t* out, int nout)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(out);
    if (nout < 8) return fail(ZC_ERR_BAD_ARG, "zc_msm_batch_plan: nout < 8");
    const Tuning& tune = ctx->devs[0].tune;
    if (int rc = msm_batch_check(n, batch, tune, "zc_msm_batch_plan")) return rc;
    if (batch == 1) {
        int32_t s[17];                                       // zc_msm_plan's entries: [7] window groups (0 below the bucket threshold)
        if (int rc = msm_plan_report(ctx, "zc_msm_batch_plan", n, points_aligned16, s)) return rc;
        const int32_t v[8] = {s[7] ? 1 : 0, s[0], s[1], s[2], s[4], s[5], s[6], s[8]};
        memcpy(out, v, sizeof v);
        return ZC_OK;
    }
    const MsmBucketPlan p = msm_batch_plan(n, batch, points_aligned16 != 0, tune.msm);
    const int32_t v[8] = {p.buckets ? 1 : 0, p.c, p.W, p.affine ? 1 : 0, p.T, p.seg, p.sort.passes, p.buckets ? p.rec_bytes : 0};
    memcpy(out, v, sizeof v);
    return ZC_OK;
}

// ---- zerocaf_hip_ext_sum.h (a part of zerocaf_hip_ext.h): the weighted sum of all rows of a wire-format batch as ONE MSM (zc_ris_batch.hip.h)
// out32 = compress(b B + sum over the accepted rows of w_ij decompress(E_ij)).  Three passes turn the bytes into ordinary MSM
// inputs in the slot's `ris_sum` workspace -- 160-byte records, canonical scalars, the base term as one more pair -- and
// msm_on_device runs on them as it stands; the one result point goes through the Ristretto encoder.  Inputs host (staged on
// device slot 0, as zc_msm_batch stages) or all on one device of the context; synchronous.
int zc_ris_lincomb_sum(zc_ctx* ctx, const uint8_t* in32, const uint64_t* scalars, size_t terms, const uint64_t* base_scalars, const uint64_t* weights,
                       uint8_t* out32, uint8_t* ok, size_t n)
{
    REQUIRE(in32); REQUIRE(scalars); REQUIRE(out32);
    if (terms == 0) return fail(ZC_ERR_BAD_ARG, "zc_ris_lincomb_sum: terms must be at least 1");
    // pairs = n terms (+ 1): 31-bit record indices, as msm_on_device requires of a shard
    if (n > (((size_t)1 << 31) - 2) / terms)
        return fail(ZC_ERR_BAD_ARG, "zc_ris_lincomb_sum: n * terms + 1 must stay below 2^31");
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    const size_t pairs = n * terms, count = pairs + (base_scalars ? 1 : 0);
    {
        // the other limits of a shard of `count` pairs, before anything is touched (msm_on_device checks the same)
        const MsmPlan mp = msm_plan(count, true, ctx->devs[0].tune.msm);
        if (mp.bad_groups) return fail(ZC_ERR_BAD_ARG, "zc_ris_lincomb_sum: ZC_MSM_GROUPS does not add up to the window count of n * terms + 1 pairs");
        if (count >= zc::MSM_BUCKET_MIN_N && zc::msm_index_limit(0, mp.m, 0))
            return fail(ZC_ERR_BAD_ARG, "zc_ris_lincomb_sum: n * terms + 1 pairs do not fit 32-bit pair indices");
    }
    if (n == 0) {
        memset(out32, 0, 32);                                    // the empty sum: the identity's encoding
        return ZC_OK;
    }
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, {in32, scalars, base_scalars, weights, ok}, "zc_ris_lincomb_sum: ", &owner)) return rc;
    {
        Residency r;
        int d = -1;
        residency_of(out32, &r, &d);
        if (r == RES_DEVICE) return fail(ZC_ERR_MIXED_MEM, "zc_ris_lincomb_sum: out32 must be host memory");
    }
    DevState& D = owner ? *owner : ctx->devs[0];
    if (int rc = ring_check(D)) return rc;
    HIP_TRY(hipSetDevice(D.device));
    const uint8_t* din = in32;
    const u64 *dk = scalars, *dkb = base_scalars, *dz = weights;
    uint8_t* dok = ok;
    if (!owner) {
        const void* src[4] = {in32, scalars, base_scalars, weights};
        const size_t bytes[5] = {pairs * 32, pairs * 40, n * 40, n * 40, n};
        for (int a = 0; a < 5; a++)
            if (a < 4 ? src[a] != nullptr : ok != nullptr)
                if (int rc = D.scratch[a].grow(bytes[a])) return rc;
        for (int a = 0; a < 4; a++)
            if (src[a]) HIP_TRY(hipMemcpyAsync(D.scratch[a].as<void>(), src[a], bytes[a], hipMemcpyHostToDevice, D.s()));
        din = D.scratch[0].as<const uint8_t>();
        dk = D.scratch[1].as<const u64>();
        if (base_scalars) dkb = D.scratch[2].as<const u64>();
        if (weights) dz = D.scratch[3].as<const u64>();
        if (ok) dok = D.scratch[4].as<uint8_t>();
    }
    // the workspace: records and scalars of `count` pairs, a flag per (row, term), t_i per row and the partial sums of the
    // base term, the 32 bytes of the result
    const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t blocks = std::min((n + zc::ZC_BLOCK * zc::SC_SUM_ROWS_PER_LANE - 1) / (zc::ZC_BLOCK * zc::SC_SUM_ROWS_PER_LANE), zc::SC_SUM_MAX_BLOCKS);
    const size_t o_k = up(count * 160), o_f = o_k + up(count * 40), o_t = o_f + up(pairs), o_p = o_t + up(base_scalars ? n * 40 : 0),
                 o_e = o_p + up(base_scalars ? blocks * 40 : 0);
    if (int rc = D.ris_sum.grow(o_e + 256)) return rc;
    char* const ws = D.ris_sum.as<char>();
    u64 *const wP = (u64*)ws, *const wK = (u64*)(ws + o_k), *const wT = base_scalars ? (u64*)(ws + o_t) : nullptr, *const wPart = (u64*)(ws + o_p);
    uint8_t *const wF = (uint8_t*)(ws + o_f), *const wE = (uint8_t*)(ws + o_e);
    hipLaunchKernelGGL(zc::k_ris_sum_prepare, dim3(grid_for(pairs)), dim3(zc::ZC_BLOCK), 0, D.s(), din, dk, dz, wP, wK, wF, terms, pairs);
    hipLaunchKernelGGL(zc::k_ris_sum_rows, dim3(grid_for(n)), dim3(zc::ZC_BLOCK), 0, D.s(), (const uint8_t*)wF, wK, dkb, dz, dok, wT,
                       base_scalars ? wP + 20 * pairs : nullptr, terms, n);
    if (base_scalars) {
        // b -> the scalar of the last pair: one workgroup's sum directly, else a partial per workgroup and one workgroup over those
        u64* const b = wK + 5 * pairs;
        hipLaunchKernelGGL(zc::k_sc_sum, dim3((unsigned)blocks), dim3(zc::ZC_BLOCK), 0, D.s(), (const u64*)wT, n, blocks == 1 ? b : wPart);
        if (blocks > 1) hipLaunchKernelGGL(zc::k_sc_sum, dim3(1), dim3(zc::ZC_BLOCK), 0, D.s(), (const u64*)wPart, blocks, b);
    }
    HIP_TRY(hipGetLastError());
    const u64* res = nullptr;
    if (int rc = msm_on_device(D, wP, wK, count, &res)) return rc;
    hipLaunchKernelGGL(zc::k_ris_compress, dim3(1), dim3(zc::ZC_BLOCK), 0, D.s(), res, wE, (size_t)1);
    HIP_TRY(hipGetLastError());
    if (!owner && ok) HIP_TRY(hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, D.s()));
    HIP_TRY(hipMemcpyAsync(out32, wE, 32, hipMemcpyDeviceToHost, D.s()));
    HIP_TRY(hipStreamSynchronize(D.s()));
    return ZC_OK;
}

// The same with the sum left in DEVICE memory (out_dev_point: 160 bytes on the device that owns
// the inputs, or on device slot 0 for host inputs); asynchronous on the context stream.
int zc_msm_partial(zc_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n, uint64_t* out_dev_point)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(out_dev_point);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState* od = nullptr;
    if (int rc = owner_of(ctx, {out_dev_point}, "", &od)) return rc;
    if (!od) return fail(ZC_ERR_MIXED_MEM, "zc_msm_partial: out_dev_point must be device memory");
    if (n == 0) {
        HIP_TRY(hipSetDevice(od->device));
        HIP_TRY(hipMemcpyAsync(out_dev_point, IDENT_POINT, 160, hipMemcpyHostToDevice, od->s()));
        HIP_TRY(hipStreamSynchronize(od->s()));           // the source is host constant memory
        return ZC_OK;
    }
    REQUIRE(points); REQUIRE(scalars);
    DevState* owner = nullptr;
    const u64* res = nullptr;
    int rc = msm_local(ctx, points, scalars, n, &owner, &res);
    if (rc) return rc;
    if (owner != od) return fail(ZC_ERR_MIXED_MEM, "zc_msm_partial: output lives on another device than the sum");
    HIP_TRY(hipSetDevice(owner->device));
    HIP_TRY(hipMemcpyAsync(out_dev_point, res, 160, hipMemcpyDeviceToDevice, owner->s()));
    return ZC_OK;
}

// ((p_0 + p_1) + p_2) + ... + p_(count-1), unified addition (src/edwards.rs:465-489), ONE launch;
// host or device pointers as everywhere.  The exchange step of a sharded MSM after an all-gather.
int zc_ed_fold_ordered(zc_ctx* ctx, const uint64_t* parts, size_t count, uint64_t* out)
{
    REQUIRE(parts); REQUIRE(out);
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    if (count == 0) return fail(ZC_ERR_BAD_ARG, "zc_ed_fold_ordered: empty list");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DevState* owner = nullptr;
    if (int rc = owner_of(ctx, {parts, out}, "", &owner)) return rc;
    DevState* ds = owner ? owner : &ctx->devs[0];
    if (int rc = ring_check(*ds)) return rc;
    HIP_TRY(hipSetDevice(ds->device));
    if (owner) {
        hipLaunchKernelGGL(zc::k_ed_fold_ordered, dim3(1), dim3(64), 0, ds->s(), (const u64*)parts, count, (const u64*)nullptr, (u64*)out);
        HIP_TRY(hipGetLastError());
        return ZC_OK;
    }
    if (int rc = ds->part.grow((count + 1) * 160)) return rc;
    u64* part = ds->part.as<u64>();
    HIP_TRY(hipMemcpyAsync(part, parts, count * 160, hipMemcpyHostToDevice, ds->s()));
    hipLaunchKernelGGL(zc::k_ed_fold_ordered, dim3(1), dim3(64), 0, ds->s(), (const u64*)part, count, (const u64*)nullptr, part + 20 * count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, part + 20 * count, 160, hipMemcpyDeviceToHost, ds->s()));
    HIP_TRY(hipStreamSynchronize(ds->s()));
    return ZC_OK;
}

// ---- one process per GPU: RCCL communicator owned by the context ------------------------------
int zc_comm_unique_id(uint8_t* id_out128)
{
    REQUIRE(id_out128);
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId id;
    RCCL_TRY(g_rccl.GetUniqueId(&id));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id_out128, &id, sizeof id);
    return ZC_OK;
}
int zc_comm_init(zc_ctx* ctx, const uint8_t* id128, int rank, int world)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(id128);
    if (world < 1 || rank < 0 || rank >= world) return fail(ZC_ERR_BAD_ARG, "zc_comm_init: bad rank / world size");
    int rc = rccl_load();
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->comm) return fail(ZC_ERR_BAD_ARG, "zc_comm_init: the context already has a communicator");
    HIP_TRY(hipSetDevice(ctx->devs[0].device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    RCCL_TRY(g_rccl.CommInitRank(&ctx->comm, world, id, rank));
    ctx->rank = rank;
    ctx->world = world;
    return ZC_OK;
}
int zc_comm_destroy(zc_ctx* ctx)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->comm) {
        (void)drain_slots_locked(ctx);
        RCCL_TRY(g_rccl.CommDestroy(ctx->comm));
        ctx->comm = nullptr;
        ctx->world = 1;
        ctx->rank = 0;
    }
    return ZC_OK;
}

// The number of ranks RCCL itself reports for the context's communicator (ncclCommCount); 0 without one.
// What a scaling record quotes to show that the exchange really ran over N ranks.
int zc_comm_size(zc_ctx* ctx, int* ranks)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(ranks);
    std::lock_guard<std::mutex> lock(ctx->mu);
    *ranks = 0;
    if (ctx->comm) RCCL_TRY(g_rccl.CommCount(ctx->comm, ranks));
    return ZC_OK;
}

// BASELINE configs[4]: this rank's shard of a global MSM.  Local bucket method -> ncclAllGather of
// the 160-byte partial sums over xGMI (20 x ncclUint64 per rank, on the context stream) -> ordered
// fold in one kernel -> every rank returns the same point (identical limbs).  Point addition is not
// an ncclRedOp_t, hence all-gather + fold rather than ncclAllReduce.
// A rank whose local part fails (bad arguments, no memory, a HIP error) still joins the collective -- with a
// poison record no point can equal (limbs of all ones) -- so that no other rank is left waiting in it; every
// rank then sees the poison among the gathered rows and ALL of them return an error.
int zc_msm_sharded(zc_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n_local, uint64_t* out_point)
{
    if (!ctx) return fail(ZC_ERR_BAD_ARG, "null context");
    REQUIRE(out_point);
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->comm) return fail(ZC_ERR_BAD_ARG, "zc_msm_sharded: call zc_comm_init first");
    DevState* d0 = &ctx->devs[0];
    const size_t world = (size_t)ctx->world;
    HIP_TRY(hipSetDevice(d0->device));
    const size_t front = ctx->devs.size() + 1;               // gather_and_fold's region (multi-slot host inputs)
    if (int rc = d0->part.grow((front + world + 2) * 160)) return rc;   // nothing to send from: the one failure that cannot join
    u64* gathered = d0->part.as<u64>() + 20 * front;
    u64* mine = gathered + 20 * world;                       // mine, then the folded result
    int local_rc = ZC_OK;
    std::string local_err;
    if (n_local == 0) {
        HIP_TRY(hipMemcpyAsync(mine, IDENT_POINT, 160, hipMemcpyHostToDevice, d0->s()));
    } else {
        DevState* owner = nullptr;
        const u64* res = nullptr;
        if (!points || !scalars) local_rc = fail(ZC_ERR_BAD_ARG, "zc_msm_sharded: null points / scalars");
        if (!local_rc) local_rc = msm_local(ctx, points, scalars, n_local, &owner, &res);
        if (!local_rc && owner != d0) local_rc = fail(ZC_ERR_MIXED_MEM, "zc_msm_sharded: inputs must live on device slot 0 (or on the host)");
        if (local_rc) local_err = g_last_error;
        HIP_TRY(hipSetDevice(d0->device));
        if (local_rc)
            HIP_TRY(hipMemsetAsync(mine, 0xFF, 160, d0->s()));
        else
            HIP_TRY(hipMemcpyAsync(mine, res, 160, hipMemcpyDeviceToDevice, d0->s()));
    }
    RCCL_TRY(g_rccl.AllGather(mine, gathered, 20, ncclUint64, ctx->comm, d0->s()));
    hipLaunchKernelGGL(zc::k_ed_fold_ordered, dim3(1), dim3(64), 0, d0->s(), (const u64*)gathered, world, (const u64*)nullptr, mine + 20);
    HIP_TRY(hipGetLastError());
    std::vector<u64> host(20 * (world + 2));                 // the gathered rows ride along: one small copy
    HIP_TRY(hipMemcpyAsync(host.data(), gathered, host.size() * sizeof(u64), hipMemcpyDeviceToHost, d0->s()));
    HIP_TRY(hipStreamSynchronize(d0->s()));
    if (local_rc) {
        g_last_error = local_err;
        return local_rc;
    }
    for (size_t r = 0; r < world; r++)
        if (host[20 * r] == ~(u64)0) return fail(ZC_ERR_HIP, ("zc_msm_sharded: rank " + std::to_string(r) + " failed its local part").c_str());
    memcpy(out_point, host.data() + 20 * (world + 1), 160);
    return ZC_OK;
}

}  // extern "C"
