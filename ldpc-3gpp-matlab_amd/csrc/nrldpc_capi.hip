// nrldpc_capi.hip -- the C ABI of include/nrldpc.h over the gfx950 kernels.
//
// Host-pointer entry points stage through device buffers owned by the handle; *_dev entry points
// launch directly on caller-owned device memory.  No CPU fallback exists anywhere in this library:
// every decode/encode is a HIP kernel launch, and any HIP failure is reported as NRLDPC_ERR_HIP.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "nrldpc.h"
#include "nrldpc_hostpath.h"
#include "nrldpc_kernels.h"
#include "nrldpc_host_quant.h"

#ifndef NRLDPC_HOST_SPIN_US_DEFAULT
#define NRLDPC_HOST_SPIN_US_DEFAULT 300 // see HostPool::spin_us
#endif
#include "nrldpc_sched.h"
#include "nrldpc_bp.h"
#include "nrldpc_cwout.h"
#include "nrldpc_modem.h"
#include "nrldpc_ratematch_ex.h"
#include "nrldpc_mix.h"
#include "nrldpc_mix_skip.h"
#include "nrldpc_mix_tx.h"
#include "nrldpc_mix_chan.h"
#include "nrldpc_mix_mc.h"
#include "nrldpc_rm_core.h"

static_assert(sizeof(nrldpc_cw_out) == 32, "nrldpc_cw_out: the size include/nrldpc.h states");

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hipfail(hipError_t e, const char* what) {
    return fail(NRLDPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return hipfail(_e, #expr); \
    } while (0)

// extern "C" bodies must not let C++ exceptions (std::bad_alloc from the staging vectors, std::system_error from the
// copy threads) cross the ABI: they become return codes.
#define NRLDPC_API_BEGIN try {
#define NRLDPC_API_END                                                                                   \
    }                                                                                                    \
    catch (const std::bad_alloc&) { return fail(NRLDPC_ERR_NOMEM, "host allocation failed"); }           \
    catch (const std::exception& ex) { return fail(NRLDPC_ERR_HIP, std::string("internal error: ") + ex.what()); } \
    catch (...) { return fail(NRLDPC_ERR_HIP, "internal error"); }

// Makes the handle's device current for the duration of a call and puts the caller's device back afterwards: a
// caller that drives several GPUs from one thread (or whose framework tracks its own current device) is not disturbed.
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev); else prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define DEVICE_SCOPE(h)                                  \
    DeviceScope _scope((h)->cfg.device_id);              \
    if (_scope.err != hipSuccess) return hipfail(_scope.err, "hipSetDevice")

template <class T> struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t reserve(size_t want) {
        if (want <= n) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// Pinned host memory for the host-pointer entry points (DMA at PCIe rate; pageable memory is not).
struct PinBuf {
    char* p = nullptr;
    size_t n = 0;
    hipError_t reserve(size_t want) {
        if (want <= n) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr; n = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault);
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
};

// A few persistent host threads that move (and quantise / narrow) the caller's pageable arrays into / out of the pinned
// staging buffers: one core does not keep up with PCIe.  On a two-socket host they have to run on the NUMA node that
// HOLDS the caller's array: threads on the other socket read it over the inter-socket links (~120 GB/s for everyone
// together, measured: 855 MB of MATLAB doubles took 7 ms however many threads there were), and the node the calling thread
// happens to run on says little about where its array was first touched.  So the pool asks the kernel where the array's
// pages are (move_pages with no target nodes = query) and moves its threads there, per call.
static int numa_cpus(std::vector<cpu_set_t>* out) { // CPUs of node 0, 1, ... (/sys/devices/system/node/node*/cpulist)
    out->clear();
    for (int node = 0; node < 64; ++node) {
        char path[96];
        snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
        FILE* f = fopen(path, "r");
        if (!f) break;
        char buf[4096];
        const bool ok = fgets(buf, sizeof buf, f) != nullptr;
        fclose(f);
        cpu_set_t set;
        CPU_ZERO(&set);
        if (ok)
            for (char* p = buf; *p && *p != '\n';) { // "0-63,128-191"
                char* e;
                const long a = strtol(p, &e, 10);
                long b = a;
                if (*e == '-') b = strtol(e + 1, &e, 10);
                for (long c = a; c <= b && c < CPU_SETSIZE; ++c) CPU_SET((int)c, &set);
                p = (*e == ',') ? e + 1 : e;
                if (e == p && *e != ',') break;
            }
        out->push_back(set);
    }
    return (int)out->size();
}

// NUMA node that holds most of [p, p + bytes) (sampled), -1 if unknown
static int numa_node_of(const void* p, size_t bytes) {
#ifdef SYS_move_pages
    const long page = sysconf(_SC_PAGESIZE);
    if (page <= 0 || bytes == 0) return -1;
    constexpr int NSAMP = 9;
    void* addr[NSAMP];
    int status[NSAMP];
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes - 1;
    for (int i = 0; i < NSAMP; ++i) {
        addr[i] = reinterpret_cast<void*>((lo + (uintptr_t)((double)(hi - lo) * i / (NSAMP - 1))) & ~(uintptr_t)(page - 1));
        status[i] = -1;
    }
    if (syscall(SYS_move_pages, 0, (unsigned long)NSAMP, addr, nullptr, status, 0) != 0) return -1;
    int votes[64] = {};
    for (int i = 0; i < NSAMP; ++i)
        if (status[i] >= 0 && status[i] < 64) ++votes[status[i]];
    int best = -1;
    for (int n = 0; n < 64; ++n)
        if (votes[n] > 0 && (best < 0 || votes[n] > votes[best])) best = n;
    return best;
#else
    (void)p; (void)bytes;
    return -1;
#endif
}

// CPUs this process may actually use: the cgroup CPU quota (v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us) when
// there is one, else what the scheduler reports.
static int usable_cpus() {
    long quota = -1, period = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
        fclose(f);
    } else {
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%ld", &quota) != 1) quota = -1; fclose(g); }
        if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%ld", &period) != 1) period = 0; fclose(g); }
    }
    const unsigned hc = std::thread::hardware_concurrency();
    int n = hc ? (int)hc : 8;
    if (quota > 0 && period > 0) n = std::min(n, (int)((quota + period - 1) / period));
    return std::max(1, n);
}

class HostPool {
    // Fork/join on every chunk of a pipelined call: a dozen jobs of 0.1-0.4 ms each within a few milliseconds.  Waking
    // sixteen sleeping threads through a condition variable costs 0.15-0.2 ms per job (measured: 13 chunks x 2 jobs made
    // 4 ms of a 12 ms call), so workers poll the generation counter for a short while after a job before they go back
    // to sleep, and the caller polls the completion counter.
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, cv_done_;
    std::function<void(int, int)> job_;
    std::atomic<int> caller_sleeps_{0};
    std::atomic<unsigned> gen_{0};
    std::atomic<int> pending_{0};
    std::atomic<int> sleepers_{0};
    std::atomic<bool> stop_{false};

    // NRLDPC_HOST_SPIN_US: how long an idle copy thread polls for the next job before it sleeps -- WHILE A CALL IS IN FLIGHT
    // (hot_: set by the chunked host path for its duration); between calls the threads sleep at once.  Waking fifteen sleeping
    // threads costs 50-150 us per job, a chunked call is 11 jobs, and round 6 measured what that adds up to: the copy / quantise
    // phase of a 4096-codeword call of doubles takes 4.4 ms with polling threads and 6.0-8.7 ms with sleeping ones (fp16: 1.0 against
    // 2.0-3.0; profiles/r06_host_copy_thread_polling.txt) -- most of what rounds 4 and 5 read as "the host's DRAM drifts".
    // Through round 5 the default was 0: a container with a CPU quota (the MI355X boxes of this build: 256 CPUs visible,
    // cpu.max = 16) charges polling like work, and a throttled process loses 20-30 ms at a time.  Polling only inside a call and
    // only for a bounded time after each job keeps that charge to the gaps between the jobs of a copy-bound call (tens of
    // microseconds each); a device-bound call's long gaps still put the threads to sleep.
    static int spin_us() {
        static const int v = getenv("NRLDPC_HOST_SPIN_US") ? atoi(getenv("NRLDPC_HOST_SPIN_US")) : NRLDPC_HOST_SPIN_US_DEFAULT;
        return v;
    }
    std::atomic<bool> hot_{false};
    static void relax() {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }

public:
    std::vector<cpu_set_t> nodes_;
    cpu_set_t proc_mask_; // affinity of the creating thread = what the host process allows
    int node_ = -1;

    explicit HostPool(int n) {
        CPU_ZERO(&proc_mask_);
        if (sched_getaffinity(0, sizeof(cpu_set_t), &proc_mask_) != 0)
            for (int c = 0; c < CPU_SETSIZE; ++c) CPU_SET(c, &proc_mask_);
        if (getenv("NRLDPC_HOST_NO_PIN") == nullptr) (void)numa_cpus(&nodes_);
        for (int i = 0; i < n; ++i)
            th_.emplace_back([this, i, n] {
                unsigned seen = 0;
                for (;;) {
                    const auto t0 = std::chrono::steady_clock::now();
                    int polls = 0;
                    while (gen_.load(std::memory_order_acquire) == seen && !stop_.load(std::memory_order_relaxed)) {
                        relax();
                        const bool hot = hot_.load(std::memory_order_relaxed);
                        if (!hot || (((++polls & 255) == 0 || spin_us() == 0) && std::chrono::steady_clock::now() - t0 >= std::chrono::microseconds(spin_us()))) {
                            std::unique_lock<std::mutex> lk(m_);
                            sleepers_.fetch_add(1);
                            cv_.wait(lk, [&] { return stop_.load() || gen_.load() != seen; });
                            sleepers_.fetch_sub(1);
                        }
                    }
                    if (stop_.load()) return;
                    seen = gen_.load(std::memory_order_acquire);
                    job_(i, n); // published before the generation moved; the next run() starts only after this one is done
                    if (pending_.fetch_sub(1, std::memory_order_acq_rel) == 1 && caller_sleeps_.load() != 0) {
                        std::lock_guard<std::mutex> lk(m_);
                        cv_done_.notify_all();
                    }
                }
            });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_.store(true);
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    // a chunked call is in flight (the workers poll between its jobs) / over (they sleep)
    void set_hot(bool on) { hot_.store(on, std::memory_order_relaxed); }
    // Run the workers on the NUMA node that holds the caller's array (no-op when it is unknown or unchanged).
    void follow(const void* p, size_t bytes) {
        if (nodes_.size() < 2) return;
        const int node = numa_node_of(p, bytes);
        if (node < 0 || node >= (int)nodes_.size() || node == node_) return;
        // never widen what the host process was started with (taskset / numactl / a MATLAB worker's mask): the workers
        // move to the node's CPUs that the process itself may run on, and stay where they are when there is none
        cpu_set_t want;
        CPU_AND(&want, &nodes_[node], &proc_mask_);
        node_ = node;
        if (CPU_COUNT(&want) == 0) return;
        for (auto& t : th_) (void)pthread_setaffinity_np(t.native_handle(), sizeof(cpu_set_t), &want);
    }
    // f(worker, nworkers) on every worker; returns when all are done
    void run(std::function<void(int, int)> f) {
        start(std::move(f));
        finish();
    }
    // the same in two halves: the caller's thread is free between them (it takes finished chunks' results out meanwhile)
    void start(std::function<void(int, int)> f) {
        job_ = std::move(f);
        pending_.store((int)th_.size(), std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(m_); // a worker between its last poll and cv_.wait holds this lock
            gen_.fetch_add(1, std::memory_order_release);
        }
        if (sleepers_.load() > 0) cv_.notify_all();
    }
    bool done() const { return pending_.load(std::memory_order_acquire) == 0; }
    void finish() {
        // poll for the usual sub-millisecond job; on an oversubscribed host (several handles decoding at once, each with
        // its own pool) give the core away instead
        const auto t0 = std::chrono::steady_clock::now();
        int polls = 0;
        while (pending_.load(std::memory_order_acquire) != 0) {
            relax();
            if (((++polls & 255) == 0 || spin_us() == 0) && std::chrono::steady_clock::now() - t0 >= std::chrono::microseconds(5 * spin_us())) {
                std::unique_lock<std::mutex> lk(m_);
                caller_sleeps_.store(1);
                cv_done_.wait_for(lk, std::chrono::milliseconds(2), [&] { return pending_.load() == 0; });
                caller_sleeps_.store(0);
            }
        }
    }
    // dst[i] = int8 grid value of src[i] (nrldpc_host_quant.h) for n elements; true when a -inf was met
    bool quantise(int8_t* dst, const void* src, size_t n, int kind, float scale) {
        std::atomic<int> neg{0};
        const size_t es = kind == NRLDPC_HQ_F64 ? 8 : kind == NRLDPC_HQ_F16 ? 2 : 4;
        run([=, &neg](int w, int nw) {
            const size_t per = ((n + nw - 1) / nw + 63) & ~(size_t)63, lo = std::min(n, per * w), hi = std::min(n, lo + per);
            if (hi > lo && nrldpc_quantise_i8(dst + lo, static_cast<const char*>(src) + lo * es, hi - lo, kind, scale))
                neg.store(1, std::memory_order_relaxed);
        });
        return neg.load() != 0;
    }
    // the same for the first `act` elements of each of n_rows rows that are `pitch` elements apart in src; dst is COMPACT
    // ([n_rows][act]); the compact range [c_lo, c_hi) only (multiples of 64 or the end) -- the rest of a row is known to be zero
    // and is neither read nor sent (nrldpc.h "Active layers")
    // (two halves, see start / finish: quantise_rows_start, then quantise_rows_finish() = "a -inf was met")
    std::atomic<int> neg_{0};
    void quantise_rows_start(int8_t* dst, const void* src, size_t act, size_t pitch, size_t c_lo, size_t c_hi, int kind, float scale) {
        neg_.store(0, std::memory_order_relaxed);
        const size_t es = kind == NRLDPC_HQ_F64 ? 8 : kind == NRLDPC_HQ_F16 ? 2 : 4, n = c_hi - c_lo;
        start([=](int w, int nw) {
            const size_t per = ((n + nw - 1) / nw + 63) & ~(size_t)63, lo = c_lo + std::min(n, per * w), hi = std::min(c_hi, lo + per);
            for (size_t pos = lo; pos < hi;) {
                const size_t r = pos / act, in_row = pos - r * act, len = std::min(hi - pos, act - in_row);
                if (nrldpc_quantise_i8(dst + pos, static_cast<const char*>(src) + (r * pitch + in_row) * es, len, kind, scale))
                    neg_.store(1, std::memory_order_relaxed);
                pos += len;
            }
        });
    }
    bool quantise_rows_finish() {
        finish();
        return neg_.load() != 0;
    }
    // NRLDPC_LAYERS_AUTO: highest block in [first, nblocks) holding anything but +-0 / NaN in any of n_cw codewords (nrldpc_host_quant.h)
    int top_block(const void* src, int kind, size_t n_cw, int Z, int nblocks, int first) {
        int best = first - 1;
        run([=, &best](int w, int nw) { nrldpc_top_block(src, kind, n_cw, (size_t)w, (size_t)nw, Z, nblocks, first, &best); });
        return best;
    }
    // dst[i] = src[i] for n bytes, or float(dst) = double(src) for n elements when narrow
    void move(void* dst, const void* src, size_t n, bool narrow) {
        run([=](int w, int nw) {
            const size_t per = ((n + nw - 1) / nw + 63) & ~(size_t)63, lo = std::min(n, per * w), hi = std::min(n, lo + per);
            if (narrow) {
                const double* d = static_cast<const double*>(src);
                float* o = static_cast<float*>(dst);
                for (size_t i = lo; i < hi; ++i) o[i] = (float)d[i];
            } else if (hi > lo) {
                memcpy(static_cast<char*>(dst) + lo, static_cast<const char*>(src) + lo, hi - lo);
            }
        });
    }
};

} // namespace

struct nrldpc_codec {
    nrldpc_cfg cfg;
    nrldpc::Schedule sched;
    float alpha = 0.75f, beta = 0.0f; // beta in LLR units; the kernels get beta*scale (the rule of `rule_layers` rows)
    int scale = 8;
    // active layers (ABI revision 5): a property of the call.  layers = what the next call uses: 4..rows, or NRLDPC_LAYERS_AUTO;
    // last_layers = what the last call ran with; rule_auto: cfg.alpha == 0, the check-node rule follows the count in use
    int layers = 0, last_layers = 0, rule_layers = 0;
    bool rule_auto = false;
    // batch counters of the parity-stop kernels that refill their codeword slots (DecArgs::work): a ring, one per launch in flight
    DevBuf<int32_t> d_work;
    unsigned work_seq = 0;
    double host_phases[10] = {}; // of the last chunked host-pointer call (nrldpc_last_host_phases); [0] = 0: none yet
    static constexpr unsigned kWorkRing = 64;
    hipEvent_t work_done[kWorkRing] = {}; // recorded behind the launch that took the slot: a slot is reused only once that launch is over
    DevBuf<int32_t> d_best; // NRLDPC_LAYERS_AUTO on device pointers: the pre-pass kernel's result ...
    PinBuf pin_best;        // ... and where the host reads it
    // device tables
    DevBuf<int32_t> d_rot;
    DevBuf<uint32_t> d_crc; // x^(crc_bits-1-i) mod g, i < crc_bits: the CRC-aided stop's table (early_term = 2)
    DevBuf<uint16_t> d_row_ptr, d_shift;
    DevBuf<uint8_t> d_col;
    // encoder solve order
    int p0_shift = 0, step_row[3] = {0, 0, 0}, step_col[3] = {0, 0, 0}, step_shift[3] = {0, 0, 0};
    int step_nk[3] = {0, 0, 0}, step_kcol[3][3] = {}, step_kshift[3][3] = {}; // already-known core blocks in that row
    // host-entry staging
    DevBuf<char> s_llr;
    DevBuf<int8_t> s_q; // int8 chunks of the pipelined host path, one region per slot
    DevBuf<uint8_t> s_hard, s_bits, s_pk; // s_pk: bit-packed hard decisions (nrldpc_decode_packed)
    DevBuf<int32_t> s_iters;
    DevBuf<float> s_app;
    std::vector<float> h_narrow;
    // argument blocks + workgroup prefix tables of nrldpc_decode_multi_dev: a ring of slots (pinned host copy, device
    // copy, completion event), so that calls in flight on different streams never share a table
    struct MultiSlot { PinBuf pin; DevBuf<char> dev; hipEvent_t done = nullptr; bool used = false; };
    static constexpr int kMultiSlots = 4;
    MultiSlot multi[kMultiSlots];
    int multi_next = 0;
    // side streams for the launches of one nrldpc_decode_multi_dev call: each launch is bound by its slowest
    // workgroups (25 iterations of a codeword that never converges), not by throughput, so the launches of the two
    // base graphs overlap almost perfectly (fork / join with events around the caller's stream)
    static constexpr int kSide = 7;
    hipStream_t side[kSide] = {};
    hipEvent_t ev_fork = nullptr, ev_join[kSide] = {};
    // pipelined host path (large batches): two pinned slots, two streams, copy threads
    static constexpr int kSlots = 4; // chunks the host may run ahead of the device
    PinBuf pin_in[kSlots], pin_out[kSlots], pin_it[kSlots];
    hipStream_t xs[2] = {nullptr, nullptr};
    hipEvent_t xdone[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    HostPool* pool = nullptr;
    int host_threads_hint = 0; // > 0: copy threads of this handle (nrldpc_pool_* shares the cores between its handles)
    // timing
    bool timing = false, have_time = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // decoding algorithm of the calls that follow (nrldpc_set_algorithm); NRLDPC_ALG_SUM_PRODUCT: nrldpc_decode_bp.hip, whose
    // column-ordered edge list (built at the first such launch) and message workspace belong to the handle.  bp_done is recorded
    // behind every sum-product launch and the next one waits for it: a second call on another stream never reuses the workspace
    // under the first
    int32_t alg = NRLDPC_ALG_MIN_SUM;
    DevBuf<uint16_t> d_bp_col; // col_ptr [ncols+1], then col_edge [nnz]
    DevBuf<float> d_bp_ws;
    hipEvent_t bp_done = nullptr;
    bool bp_used = false;
    // nrldpc_decode_cw[_dev] on a min-sum handle: the soft output of one chunk (at most NRLDPC_CW_SCRATCH_BYTES), which the finish
    // kernel (nrldpc_cwout.hip) reads.  cw_done is recorded behind every such call and the next one waits for it, as bp_done
    DevBuf<float> d_cw_app;
    hipEvent_t cw_done = nullptr;
    bool cw_used = false;
    DevBuf<uint8_t> s_cw, s_chk; // host-entry staging of nrldpc_decode_cw
    DevBuf<int32_t> s_unsat;
};

namespace {

size_t llr_elem_bytes(int dtype) { return dtype == NRLDPC_LLR_F16 ? 2 : 4; }

// Substitution order for the core-parity blocks (same derivation as the oracle's encode_one, from the
// dual-diagonal entries at get_3gpp_base_graph.m:30-31,48-50,68-69,87-88 / :339-340,349-350,356-358,367-368).
// `shift`: the table's shifts reduced mod Z, per base-graph edge.  Fills *o (zeroed first: entries past step_nk stay 0).
bool derive_encoder_order(const nrldpc::BaseGraph& g, const int32_t* shift, nrldpc::EncSolveOrder* o) {
    *o = nrldpc::EncSolveOrder{};
    const int kb = g.kb;
    int cnt[4] = {0, 0, 0, 0}, sh0[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i)
        for (int e = g.row_ptr[i]; e < g.row_ptr[i + 1]; ++e)
            if (g.col[e] == kb) { cnt[i] = 1; sh0[i] = shift[e]; }
    int a = -1;
    for (int i = 0; i < 4; ++i) {
        if (!cnt[i]) continue;
        int n = 0;
        for (int k = 0; k < 4; ++k) n += (cnt[k] && sh0[k] == sh0[i]);
        if (n & 1) a = sh0[i];
    }
    if (a < 0) return false;
    o->p0_shift = a;
    bool known[4] = {true, false, false, false};
    for (int st = 0; st < 3; ++st) {
        bool found = false;
        for (int i = 0; i < 4 && !found; ++i) {
            int unk = -1, nunk = 0, ush = 0;
            for (int e = g.row_ptr[i]; e < g.row_ptr[i + 1]; ++e) {
                int c = g.col[e] - kb;
                if (c >= 0 && c < 4 && !known[c]) { unk = c; ush = shift[e]; ++nunk; }
            }
            if (nunk == 1) {
                o->step_row[st] = i; o->step_col[st] = unk; o->step_shift[st] = ush;
                int nk = 0;
                for (int e = g.row_ptr[i]; e < g.row_ptr[i + 1]; ++e) {
                    const int c = g.col[e] - kb;
                    if (c >= 0 && c < 4 && c != unk) {
                        if (nk == 3) return false;
                        o->step_kcol[st][nk] = c; o->step_kshift[st][nk] = shift[e]; ++nk;
                    }
                }
                o->step_nk[st] = nk;
                known[unk] = true; found = true;
            }
        }
        if (!found) return false;
    }
    return true;
}

// the handle's copy of the same values
bool derive_encoder_order(nrldpc_codec* h) {
    nrldpc::EncSolveOrder o;
    if (!derive_encoder_order(h->sched.g, h->sched.shift.data(), &o)) return false;
    h->p0_shift = o.p0_shift;
    for (int st = 0; st < 3; ++st) {
        h->step_row[st] = o.step_row[st]; h->step_col[st] = o.step_col[st]; h->step_shift[st] = o.step_shift[st];
        h->step_nk[st] = o.step_nk[st];
        for (int k = 0; k < 3; ++k) { h->step_kcol[st][k] = o.step_kcol[st][k]; h->step_kshift[st][k] = o.step_kshift[st][k]; }
    }
    return true;
}

void begin_timing(nrldpc_codec* h, hipStream_t s) {
    if (h->timing) (void)hipEventRecord(h->ev0, s);
}
void end_timing(nrldpc_codec* h, hipStream_t s) {
    if (h->timing) { (void)hipEventRecord(h->ev1, s); h->have_time = true; }
}

// the check-node rule of a call that decodes nl rows: the handle's own (explicit cfg.alpha), or -- cfg.alpha == 0 -- the library's
// rule for that count, on the grid nrldpc_create puts beta on
void rule_for(const nrldpc_codec* h, int nl, float* alpha, float* beta) {
    *alpha = h->alpha; *beta = h->beta;
    if (!h->rule_auto || nl == h->rule_layers) return;
    float a, b;
    nrldpc::default_rule(h->sched.g.bg, nl, &a, &b);
    *alpha = a;
    *beta = std::nearbyint(2.0f * b * (float)h->scale) / (2.0f * (float)h->scale);
}

// rows a block index found by the NRLDPC_LAYERS_AUTO scans stands for: block c >= kb + 4 is row c - kb's extension column
int layers_of_block(const nrldpc::Schedule& s, int top) { return std::max(4, top - s.g.kb + 1); }

// nl: active layer count of this call (4..rows, resolved by the caller)
nrldpc::DecArgs make_dec_args(const nrldpc_codec* h, const void* d_llr, int batch, uint8_t* d_hard, int32_t* d_iters,
                              float* d_app, int nl, int llr_kind = -1) {
    const nrldpc::Schedule& s = h->sched;
    nrldpc::DecArgs a;
    memset(&a, 0, sizeof a);
    a.llr = d_llr; a.hard = d_hard; a.iters = d_iters; a.app = d_app;
    a.rot = h->d_rot.p;
    a.batch = batch; a.Z = s.Z; a.n_layers = nl; a.max_iter = h->cfg.max_iter; a.ncw = s.ncw; a.sbw = s.sbw;
    a.early_term = h->cfg.early_term ? 1 : 0;
    if (h->cfg.early_term == 2) { a.crc_tab = h->d_crc.p; a.crc_bits = h->cfg.crc_bits; }
    a.need_ext = (a.early_term || d_app) ? 1 : 0;
    a.llr_kind = llr_kind >= 0 ? llr_kind : (h->cfg.llr_dtype == NRLDPC_LLR_F16) ? NRLDPC_K_F16 : NRLDPC_K_F32;
    float alpha, beta;
    rule_for(h, nl, &alpha, &beta);
    a.alpha = alpha; a.scale = (float)h->scale; a.inv_scale = 1.0f / (float)h->scale;
    a.beta = beta * (float)h->scale;
    return a;
}

// NRLDPC_LAYERS_AUTO on device pointers, first half: the pre-pass kernel over `batch` codewords at d_llr and the copy of its
// result into the handle's pinned word, all on `stream`; the caller synchronises the stream and calls auto_layers_read
int auto_layers_enqueue(nrldpc_codec* h, const void* d_llr, int batch, hipStream_t stream, int llr_kind = -1) {
    const nrldpc::Schedule& s = h->sched;
    HIP_TRY(h->d_best.reserve(1));
    HIP_TRY(h->pin_best.reserve(64));
    const int first = s.g.kb + 4, kind = llr_kind >= 0 ? llr_kind : (h->cfg.llr_dtype == NRLDPC_LLR_F16) ? NRLDPC_K_F16 : NRLDPC_K_F32;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->d_best.p), first - 1, 1, stream));
    HIP_TRY(nrldpc::launch_top_block(d_llr, kind, batch, s.Z, s.g.ncols, first, h->d_best.p, stream));
    HIP_TRY(hipMemcpyAsync(h->pin_best.p, h->d_best.p, 4, hipMemcpyDeviceToHost, stream));
    return NRLDPC_OK;
}
int auto_layers_read(const nrldpc_codec* h) { return layers_of_block(h->sched, *reinterpret_cast<const int32_t*>(h->pin_best.p)); }

// the layer count of a device-pointer call: the handle's, or -- NRLDPC_LAYERS_AUTO -- read off the data (synchronises `stream`)
int resolve_layers_dev(nrldpc_codec* h, const void* d_llr, int batch, hipStream_t stream, int* nl) {
    if (h->layers != NRLDPC_LAYERS_AUTO) { *nl = h->layers; return NRLDPC_OK; }
    int rc = auto_layers_enqueue(h, d_llr, batch, stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    *nl = auto_layers_read(h);
    return NRLDPC_OK;
}

// The batch counter of the next parity-stop launch (the persistent kernels' "next codeword", nrldpc_decode_z64p.h), from a ring of
// 64 per handle.  A slot carries an event recorded behind the launch that used it; a slot whose launch is still running -- more than
// 64 refilling launches in flight over several streams -- is NOT reset under it: this launch then runs without refilling
// (null: every workgroup decodes its own codewords), as it does when the ring cannot be allocated.
int32_t* next_work(nrldpc_codec* h, unsigned* slot) {
    if (h->d_work.reserve(nrldpc_codec::kWorkRing) != hipSuccess) return nullptr;
    const unsigned i = h->work_seq % nrldpc_codec::kWorkRing;
    if (h->work_done[i] && hipEventQuery(h->work_done[i]) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (!h->work_done[i] && hipEventCreateWithFlags(&h->work_done[i], hipEventDisableTiming) != hipSuccess) { h->work_done[i] = nullptr; return nullptr; }
    ++h->work_seq;
    *slot = i;
    return h->d_work.p + i;
}

// A sum-product launch (NRLDPC_ALG_SUM_PRODUCT) of `batch` codewords at d_llr, nl active rows: f32 or f16 LLRs as they are (no
// int8 grid, no llr_scale; alpha and beta are not read).  Persistent workgroups, as many as the device holds at once, each with its
// slice of the handle's workspace; ordered behind the handle's previous sum-product launch, whatever its stream.
// cw (nullable): nrldpc_cw_out of the call, device pointers -- written by the kernel's output stage
int bp_launch(nrldpc_codec* h, const void* d_llr, int batch, uint8_t* d_hard, int32_t* d_iters, float* d_app, hipStream_t stream,
              int nl, int llr_kind, const nrldpc_cw_out* cw = nullptr) {
    const nrldpc::Schedule& s = h->sched;
    const nrldpc::BaseGraph& g = s.g;
    if (!h->d_bp_col.p) { // column-ordered edge list, ascending edge (= row) order within a column
        std::vector<uint16_t> tab((size_t)g.ncols + 1 + g.nnz, 0);
        uint16_t* cp = tab.data();
        uint16_t* ce = cp + g.ncols + 1;
        for (int e = 0; e < g.nnz; ++e) ++cp[g.col[e] + 1];
        for (int c = 0; c < g.ncols; ++c) cp[c + 1] += cp[c];
        std::vector<uint16_t> fill(cp, cp + g.ncols);
        for (int e = 0; e < g.nnz; ++e) ce[fill[g.col[e]]++] = (uint16_t)e;
        HIP_TRY(h->d_bp_col.reserve(tab.size()));
        HIP_TRY(hipMemcpy(h->d_bp_col.p, tab.data(), tab.size() * 2, hipMemcpyHostToDevice));
    }
    if (!h->bp_done) HIP_TRY(hipEventCreateWithFlags(&h->bp_done, hipEventDisableTiming));
    const int threads = nrldpc::bp_threads(g.ncols, s.Z);
    const size_t lds = nrldpc::bp_lds_bytes(g.ncols, s.Z) + (cw ? nrldpc::CW_LDS_BYTES : 0);
    int resident = 1;
    const char* what = "";
    if (hipError_t e = nrldpc::bp_resident(threads, lds, &resident, &what)) return hipfail(e, what);
    const int grid = std::max(1, std::min(batch, resident));
    const size_t stride = ((size_t)(g.nnz + g.ncols) * s.Z + 63) & ~(size_t)63;
    if (h->d_bp_ws.n < stride * grid && h->bp_used) HIP_TRY(hipEventSynchronize(h->bp_done)); // the old workspace is freed below
    HIP_TRY(h->d_bp_ws.reserve(stride * grid));
    if (h->bp_used) HIP_TRY(hipStreamWaitEvent(stream, h->bp_done, 0));
    nrldpc::BpArgs a;
    memset(&a, 0, sizeof a);
    a.llr = d_llr; a.hard = d_hard; a.iters = d_iters; a.app = d_app;
    if (cw) { a.cw_packed = cw->cw_packed; a.unsatisfied = cw->unsatisfied; a.checks_packed = cw->checks_packed; }
    a.row_ptr = h->d_row_ptr.p; a.col = h->d_col.p; a.shift = h->d_shift.p;
    a.col_ptr = h->d_bp_col.p; a.col_edge = h->d_bp_col.p + g.ncols + 1;
    a.ws = h->d_bp_ws.p; a.ws_stride = stride;
    a.batch = batch; a.Z = s.Z; a.nrows = g.nrows; a.ncols = g.ncols; a.kb = g.kb; a.nnz = g.nnz;
    a.n_layers = nl; a.max_iter = h->cfg.max_iter; a.early_term = h->cfg.early_term ? 1 : 0;
    a.llr_f16 = (llr_kind >= 0 ? llr_kind : (h->cfg.llr_dtype == NRLDPC_LLR_F16) ? NRLDPC_K_F16 : NRLDPC_K_F32) == NRLDPC_K_F16;
    a.r_cap = (float)(2.0 * std::atanh(1.0 - 1e-15));
    h->last_layers = nl;
    begin_timing(h, stream);
    hipError_t e = nrldpc::launch_bp_flood(a, grid, threads, lds, stream);
    end_timing(h, stream);
    if (e != hipSuccess) return hipfail(e, "sum-product decode kernel launch");
    HIP_TRY(hipEventRecord(h->bp_done, stream));
    h->bp_used = true;
    return NRLDPC_OK;
}

int decode_launch(nrldpc_codec* h, const void* d_llr, int batch, uint8_t* d_hard, int32_t* d_iters, float* d_app,
                  hipStream_t stream, int nl, int llr_kind = -1) {
    if (h->alg == NRLDPC_ALG_SUM_PRODUCT) return bp_launch(h, d_llr, batch, d_hard, d_iters, d_app, stream, nl, llr_kind);
    const nrldpc::Schedule& s = h->sched;
    nrldpc::DecArgs a = make_dec_args(h, d_llr, batch, d_hard, d_iters, d_app, nl, llr_kind);
    h->last_layers = nl;
    unsigned wslot = 0;
    a.work = a.early_term ? next_work(h, &wslot) : nullptr; // only the parity-stop kernels refill
    begin_timing(h, stream);
    hipError_t e = nrldpc::launch_decode(s.g.bg, a, s.threads, s.lds_bytes, stream);
    end_timing(h, stream);
    if (a.work) (void)hipEventRecord(h->work_done[wslot], stream);
    if (e != hipSuccess) return hipfail(e, "decode kernel launch");
    return NRLDPC_OK;
}

// nrldpc_decode_cw_dev behind its argument checks: `batch` codewords at d_llr (device; llr_kind as decode_launch) with the outputs
// of *out (device pointers).  Sum-product: one launch, the kernel writes them.  Min-sum: chunks of the soft-output route into the
// handle's scratch, each followed by the finish kernel on the same stream.
int decode_cw_launch(nrldpc_codec* h, const void* d_llr, int batch, uint8_t* d_hard, int32_t* d_iters, const nrldpc_cw_out* out,
                     hipStream_t stream) {
    const nrldpc::Schedule& s = h->sched;
    const nrldpc::BaseGraph& g = s.g;
    int nl = 0;
    int rc = resolve_layers_dev(h, d_llr, batch, stream, &nl); // NRLDPC_LAYERS_AUTO: once, over the whole batch
    if (rc) return rc;
    if (h->alg == NRLDPC_ALG_SUM_PRODUCT) return bp_launch(h, d_llr, batch, d_hard, d_iters, nullptr, stream, nl, -1, out);
    const size_t N = (size_t)g.ncols * s.Z, K = (size_t)g.kb * s.Z, eb = llr_elem_bytes(h->cfg.llr_dtype);
    const size_t cbytes = ((size_t)g.nrows * s.Z + 7) / 8;
    const int chunk = (int)std::min<size_t>((size_t)batch, (size_t)NRLDPC_CW_SCRATCH_BYTES / (4 * N));
    if (!h->cw_done) HIP_TRY(hipEventCreateWithFlags(&h->cw_done, hipEventDisableTiming));
    if (h->d_cw_app.n < (size_t)chunk * N && h->cw_used) HIP_TRY(hipEventSynchronize(h->cw_done)); // the old scratch is freed below
    HIP_TRY(h->d_cw_app.reserve((size_t)chunk * N));
    if (h->cw_used) HIP_TRY(hipStreamWaitEvent(stream, h->cw_done, 0));
    for (int c0 = 0; c0 < batch; c0 += chunk) {
        const int n = std::min(chunk, batch - c0);
        rc = decode_launch(h, static_cast<const char*>(d_llr) + (size_t)c0 * N * eb, n, d_hard + (size_t)c0 * K, d_iters ? d_iters + c0 : nullptr,
                           h->d_cw_app.p, stream, nl);
        if (rc) break;
        nrldpc::CwFinishArgs a;
        memset(&a, 0, sizeof a);
        a.app = h->d_cw_app.p;
        a.cw_packed = out->cw_packed ? out->cw_packed + (size_t)c0 * ((N + 7) / 8) : nullptr;
        a.unsatisfied = out->unsatisfied ? out->unsatisfied + c0 : nullptr;
        a.checks_packed = out->checks_packed ? out->checks_packed + (size_t)c0 * cbytes : nullptr;
        a.row_ptr = h->d_row_ptr.p; a.col = h->d_col.p; a.shift = h->d_shift.p;
        a.batch = n; a.Z = s.Z; a.nrows = g.nrows; a.ncols = g.ncols; a.nnz = g.nnz; a.n_layers = nl;
        if (hipError_t e = nrldpc::launch_cw_finish(a, stream)) { rc = hipfail(e, "codeword finish kernel launch"); break; }
    }
    // recorded on failure too: whatever was queued still owns the scratch
    if (hipEventRecord(h->cw_done, stream) == hipSuccess) h->cw_used = true;
    return rc;
}

// the argument checks nrldpc_decode_cw and nrldpc_decode_cw_dev share
int check_cw_args(nrldpc_codec* h, const void* llr, int batch, const uint8_t* hard, const nrldpc_cw_out* out) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    if (batch < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (!out) return fail(NRLDPC_ERR_ARG, "null nrldpc_cw_out");
    if (out->struct_size != (uint32_t)sizeof(nrldpc_cw_out))
        return fail(NRLDPC_ERR_ARG, "nrldpc_cw_out.struct_size does not match this library (set it to sizeof(nrldpc_cw_out))");
    if (!out->cw_packed && !out->unsatisfied && !out->checks_packed)
        return fail(NRLDPC_ERR_ARG, "nrldpc_cw_out: at least one of cw_packed, unsatisfied, checks_packed must be given");
    if (h->cfg.early_term == 2)
        return fail(NRLDPC_ERR_UNSUPPORTED, "whole-codeword outputs are not available with the CRC-aided stop (early_term = 2)");
    if (batch > 0 && (!llr || !hard)) return fail(NRLDPC_ERR_ARG, "null llr/hard pointer");
    return NRLDPC_OK;
}

int encode_launch(nrldpc_codec* h, const uint8_t* d_info, int batch, uint8_t* d_cw, hipStream_t stream) {
    const nrldpc::Schedule& s = h->sched;
    nrldpc::EncArgs a;
    a.info = d_info; a.cw = d_cw;
    a.row_ptr = h->d_row_ptr.p; a.col = h->d_col.p; a.shift = h->d_shift.p;
    a.batch = batch; a.Z = s.Z; a.nrows = s.g.nrows; a.ncols = s.g.ncols; a.kb = s.g.kb; a.nnz = s.g.nnz;
    a.p0_shift = h->p0_shift;
    for (int i = 0; i < 3; ++i) {
        a.step_row[i] = h->step_row[i]; a.step_col[i] = h->step_col[i]; a.step_shift[i] = h->step_shift[i];
        a.step_nk[i] = h->step_nk[i];
        for (int k = 0; k < 3; ++k) { a.step_kcol[i][k] = h->step_kcol[i][k]; a.step_kshift[i][k] = h->step_kshift[i][k]; }
    }
    begin_timing(h, stream);
    hipError_t e = nrldpc::launch_encode(a, stream);
    end_timing(h, stream);
    if (e != hipSuccess) return hipfail(e, "encode kernel launch");
    return NRLDPC_OK;
}

// the per-code-block part of the rate-recovery arguments (RmArgs / RmExArgs: the same fields under the same names)
template <class A> int fill_rm_blocks(const nrldpc_tb_params* p, int32_t n_tb, A& a) {
    a.n_tb = n_tb; a.C = p->C; a.G = p->G; a.Z = p->Z; a.K = p->K; a.Kp = p->K_prime; a.N = p->N; a.N_cb = p->N_cb;
    a.k0 = p->k_0; a.Qm = p->Q_m;
    int off = 0;
    for (int r = 0; r < p->C; ++r) {
        if (p->E_r[r] < 0 || p->E_r[r] % p->Q_m) return fail(NRLDPC_ERR_UNSUPPORTED, "E_r must be a non-negative multiple of Q_m");
        a.E[r] = p->E_r[r]; a.off[r] = off; off += p->E_r[r];
    }
    if (off != p->G) return fail(NRLDPC_ERR_ARG, "sum(E_r) must equal G");
    return NRLDPC_OK;
}

} // namespace

extern "C" {

int nrldpc_set_index(int32_t Z) { return nrldpc::set_index(Z); }
int nrldpc_lifting_size(int32_t K_b, int32_t K_prime) { return nrldpc::lifting_size(K_b, K_prime); }

const char* nrldpc_strerror(int code) {
    switch (code) {
        case NRLDPC_OK: return "ok";
        case NRLDPC_ERR_UNSUPPORTED: return "unsupported parameters";
        case NRLDPC_ERR_ARG: return "invalid argument";
        case NRLDPC_ERR_HIP: return "HIP runtime error";
        case NRLDPC_ERR_NOMEM: return "out of memory";
        default: return "unknown error";
    }
}
const char* nrldpc_last_error(void) { return g_err.c_str(); }
const char* nrldpc_version(void) { return "nrldpc-hip 0.3 (gfx950)"; }
int nrldpc_abi_version(void) { return NRLDPC_ABI_VERSION; }
#ifndef NRLDPC_BUILD_ID
#define NRLDPC_BUILD_ID "unknown"
#endif
const char* nrldpc_build_id(void) { return NRLDPC_BUILD_ID; }
#ifndef NRLDPC_KERNEL_ID
#define NRLDPC_KERNEL_ID "unknown"
#endif
const char* nrldpc_kernel_id(void) { return NRLDPC_KERNEL_ID; }

int nrldpc_default_rule(int32_t bg, int32_t n_layers, float* alpha, float* beta) {
    if (bg != 1 && bg != 2) return fail(NRLDPC_ERR_UNSUPPORTED, "BG must be 1 or 2");
    const int rows = bg == 1 ? NR_BG1_ROWS : NR_BG2_ROWS;
    if (n_layers == 0) n_layers = rows;
    if (n_layers < 4 || n_layers > rows) return fail(NRLDPC_ERR_UNSUPPORTED, "n_layers must be 0 or in 4..rows of the base graph");
    float a, b;
    nrldpc::default_rule(bg, n_layers, &a, &b);
    if (alpha) *alpha = a;
    if (beta) *beta = b;
    return NRLDPC_OK;
}

int nrldpc_create(const nrldpc_cfg* cfg_in, nrldpc_handle* out) {
    NRLDPC_API_BEGIN
    if (!cfg_in || !out) return fail(NRLDPC_ERR_ARG, "null cfg/out");
    *out = nullptr;
    // struct_size is the caller's sizeof(nrldpc_cfg): a caller built against another revision of the header is refused
    // instead of having fields read past the end of its struct
    if (cfg_in->struct_size != (uint32_t)sizeof(nrldpc_cfg))
        return fail(NRLDPC_ERR_ARG, "nrldpc_cfg.struct_size does not match this library (set it to sizeof(nrldpc_cfg); ABI revision mismatch?)");
    const nrldpc_cfg* cfg = cfg_in;
    if (cfg->bg != 1 && cfg->bg != 2) return fail(NRLDPC_ERR_UNSUPPORTED, "BG must be 1 or 2");
    if (nrldpc::set_index(cfg->Z) < 0) return fail(NRLDPC_ERR_UNSUPPORTED, "Invalid lifting size.");
    if (cfg->max_iter < 1 || cfg->max_iter > 2000) return fail(NRLDPC_ERR_UNSUPPORTED, "max_iter must be in 1..2000");
    if (cfg->llr_dtype < NRLDPC_LLR_F32 || cfg->llr_dtype > NRLDPC_LLR_F64)
        return fail(NRLDPC_ERR_UNSUPPORTED, "unknown llr_dtype");
    float alpha = cfg->alpha, beta = cfg->beta;
    const int rows = cfg->bg == 1 ? NR_BG1_ROWS : NR_BG2_ROWS;
    if (cfg->n_layers != NRLDPC_LAYERS_ALL && cfg->n_layers != NRLDPC_LAYERS_AUTO && (cfg->n_layers < 4 || cfg->n_layers > rows))
        return fail(NRLDPC_ERR_UNSUPPORTED, "n_layers must be 0 (all), NRLDPC_LAYERS_AUTO or in 4..rows of the base graph");
    const int rows0 = cfg->n_layers > 0 ? cfg->n_layers : rows; // under NRLDPC_LAYERS_AUTO: until the first call says otherwise
    if (alpha == 0.0f) // the caller leaves the check-node rule to the library: by rate (see nrldpc_default_rule)
        nrldpc::default_rule(cfg->bg, rows0, &alpha, &beta);
    if (!(alpha > 0.0f && alpha <= 1.0f)) return fail(NRLDPC_ERR_UNSUPPORTED, "alpha must be in (0,1]");
    if (!(beta >= 0.0f && beta <= 4.0f)) return fail(NRLDPC_ERR_UNSUPPORTED, "beta must be in [0,4] LLR units");
    if (cfg->early_term < 0 || cfg->early_term > 2) return fail(NRLDPC_ERR_UNSUPPORTED, "early_term must be 0, 1 or 2");
    if (cfg->early_term == 2) { // CRC-aided stop: generator with its x^L term, L = 6 ... 24, over the first crc_bits information bits
        const int kb = cfg->bg == 1 ? 22 : 10;
        if (cfg->crc_len < 6 || cfg->crc_len > 24 || (cfg->crc_poly >> cfg->crc_len) != 1u || !(cfg->crc_poly & 1u))
            return fail(NRLDPC_ERR_UNSUPPORTED, "early_term = 2 needs crc_poly = the generator with its x^crc_len and x^0 terms, crc_len in 6..24");
        if (cfg->crc_bits <= cfg->crc_len || cfg->crc_bits > kb * cfg->Z)
            return fail(NRLDPC_ERR_UNSUPPORTED, "early_term = 2 needs crc_len < crc_bits <= K (payload and CRC of one code block)");
    }
    int scale = cfg->llr_scale == 0 ? 8 : cfg->llr_scale;
    if (scale != 1 && scale != 2 && scale != 4 && scale != 8 && scale != 16 && scale != 32)
        return fail(NRLDPC_ERR_UNSUPPORTED, "llr_scale must be a power of two in 1..32");
    nrldpc_codec* h = new (std::nothrow) nrldpc_codec();
    if (!h) return fail(NRLDPC_ERR_NOMEM, "host allocation failed");
    h->cfg = *cfg;
    h->alpha = alpha;
    // the offset lives on a grid of half fixed-point units (1/(2*llr_scale) LLR): the pipelined kernels round
    // alpha*m - beta inside one fused multiply-add against 2^23 - beta*scale, which has to be exact
    h->beta = std::nearbyint(2.0f * beta * (float)scale) / (2.0f * (float)scale);
    h->scale = scale;
    h->rule_auto = cfg->alpha == 0.0f;
    h->rule_layers = rows0;
    h->layers = cfg->n_layers == NRLDPC_LAYERS_AUTO ? NRLDPC_LAYERS_AUTO : rows0;
    if (!nrldpc::build_schedule(cfg->bg, cfg->Z, rows0, &h->sched)) {
        delete h;
        return fail(NRLDPC_ERR_UNSUPPORTED, "n_layers must be 0 (all), NRLDPC_LAYERS_AUTO or in 4..rows of the base graph");
    }
    if (!derive_encoder_order(h)) {
        delete h;
        return fail(NRLDPC_ERR_UNSUPPORTED, "base graph core is not dual-diagonal");
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        delete h;
        return fail(NRLDPC_ERR_HIP, "no HIP device available (this library has no CPU path)");
    }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) {
        delete h;
        return fail(NRLDPC_ERR_ARG, "device_id out of range");
    }
#define CREATE_TRY(expr)                                                  \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) { int rc = hipfail(_e, #expr); nrldpc_destroy(h); return rc; } \
    } while (0)
    DeviceScope scope(cfg->device_id); // the caller's current device is restored on return
    CREATE_TRY(scope.err);
    const nrldpc::Schedule& s = h->sched;
    CREATE_TRY(h->d_rot.reserve(s.rot.size()));
    CREATE_TRY(hipMemcpy(h->d_rot.p, s.rot.data(), s.rot.size() * 4, hipMemcpyHostToDevice));
    std::vector<uint16_t> sh16(s.shift.begin(), s.shift.end());
    CREATE_TRY(h->d_row_ptr.reserve(s.g.nrows + 1));
    CREATE_TRY(h->d_col.reserve(s.g.nnz));
    CREATE_TRY(h->d_shift.reserve(s.g.nnz));
    CREATE_TRY(hipMemcpy(h->d_row_ptr.p, s.g.row_ptr, (s.g.nrows + 1) * 2, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_col.p, s.g.col, s.g.nnz, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_shift.p, sh16.data(), s.g.nnz * 2, hipMemcpyHostToDevice));
    if (cfg->early_term == 2) {
        // tab[i] = x^(n-1-i) mod g: bit i of the block (first bit = highest power, as comm.CRCDetector reads it,
        // NRLDPCDecoder.m:113-115) contributes this to the remainder; built from the last bit backwards by x -> x*x mod g
        const int n = cfg->crc_bits, L = cfg->crc_len;
        std::vector<uint32_t> tab((size_t)n);
        uint32_t r = 1u; // x^0
        const uint32_t top = 1u << L;
        for (int i = n - 1; i >= 0; --i) {
            tab[(size_t)i] = r;
            r <<= 1;
            if (r & top) r ^= cfg->crc_poly;
        }
        CREATE_TRY(h->d_crc.reserve((size_t)n));
        CREATE_TRY(hipMemcpy(h->d_crc.p, tab.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        h->sched.lds_bytes += 4 * (size_t)nrldpc::CRC_SLOTS * h->sched.ncw + 16; // the run-time-Z kernel's slots, behind its flags
    }
    CREATE_TRY(hipEventCreate(&h->ev0));
    CREATE_TRY(hipEventCreate(&h->ev1));
#undef CREATE_TRY
    *out = h;
    return NRLDPC_OK;
    NRLDPC_API_END
}

void nrldpc_destroy(nrldpc_handle h) {
    if (!h) return;
    DeviceScope scope(h->cfg.device_id);
    h->d_rot.release(); h->d_crc.release(); h->d_best.release(); h->pin_best.release(); h->d_work.release();
    h->d_row_ptr.release(); h->d_col.release(); h->d_shift.release();
    h->d_bp_col.release(); h->d_bp_ws.release();
    if (h->bp_done) (void)hipEventDestroy(h->bp_done);
    h->d_cw_app.release(); h->s_cw.release(); h->s_chk.release(); h->s_unsat.release();
    if (h->cw_done) (void)hipEventDestroy(h->cw_done);
    h->s_llr.release(); h->s_q.release(); h->s_hard.release(); h->s_bits.release(); h->s_pk.release(); h->s_iters.release(); h->s_app.release();
    for (auto& m : h->multi) { m.pin.release(); m.dev.release(); if (m.done) (void)hipEventDestroy(m.done); }
    for (int i = 0; i < nrldpc_codec::kSide; ++i) {
        if (h->side[i]) (void)hipStreamDestroy(h->side[i]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (auto ev : h->work_done)
        if (ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < nrldpc_codec::kSlots; ++i) {
        h->pin_in[i].release(); h->pin_out[i].release(); h->pin_it[i].release();
        if (h->xdone[i]) (void)hipEventDestroy(h->xdone[i]);
    }
    for (int i = 0; i < 2; ++i)
        if (h->xs[i]) (void)hipStreamDestroy(h->xs[i]);
    delete h->pool;
    delete h;
}

int nrldpc_get_dims(nrldpc_handle h, nrldpc_dims* out) {
    if (!h || !out) return fail(NRLDPC_ERR_ARG, "null handle/out");
    if (out->struct_size != (uint32_t)sizeof(nrldpc_dims))
        return fail(NRLDPC_ERR_ARG, "nrldpc_dims.struct_size does not match this library (set it to sizeof(nrldpc_dims) before the call)");
    const nrldpc::Schedule& s = h->sched;
    out->nrows = s.g.nrows; out->ncols = s.g.ncols; out->kb = s.g.kb; out->i_ls = s.ils;
    out->K = s.g.kb * s.Z; out->N_cw = s.g.ncols * s.Z; out->n_layers = h->layers;
    rule_for(h, h->layers != NRLDPC_LAYERS_AUTO ? h->layers : h->last_layers ? h->last_layers : s.g.nrows, &out->alpha, &out->beta);
    return NRLDPC_OK;
}

int nrldpc_set_layers(nrldpc_handle h, int32_t n_layers) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    const int rows = h->sched.g.nrows;
    if (n_layers == NRLDPC_LAYERS_AUTO) h->layers = NRLDPC_LAYERS_AUTO;
    else if (n_layers == NRLDPC_LAYERS_ALL) h->layers = rows;
    else if (n_layers >= 4 && n_layers <= rows) h->layers = n_layers;
    else return fail(NRLDPC_ERR_UNSUPPORTED, "n_layers must be 0 (all), NRLDPC_LAYERS_AUTO or in 4..rows of the base graph");
    return NRLDPC_OK;
}

int nrldpc_set_algorithm(nrldpc_handle h, int32_t algorithm) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    if (algorithm != NRLDPC_ALG_MIN_SUM && algorithm != NRLDPC_ALG_SUM_PRODUCT) return fail(NRLDPC_ERR_UNSUPPORTED, "unknown decoding algorithm");
    if (algorithm == NRLDPC_ALG_SUM_PRODUCT && h->cfg.early_term == 2)
        return fail(NRLDPC_ERR_UNSUPPORTED, "the CRC-aided stop (early_term = 2) is not available with sum-product decoding");
    h->alg = algorithm;
    return NRLDPC_OK;
}

int nrldpc_get_algorithm(nrldpc_handle h, int32_t* algorithm) {
    if (!h || !algorithm) return fail(NRLDPC_ERR_ARG, "null handle/out");
    *algorithm = h->alg;
    return NRLDPC_OK;
}

int nrldpc_set_llr_dtype(nrldpc_handle h, int32_t llr_dtype) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    if (llr_dtype < NRLDPC_LLR_F32 || llr_dtype > NRLDPC_LLR_F64) return fail(NRLDPC_ERR_UNSUPPORTED, "unknown llr_dtype");
    h->cfg.llr_dtype = llr_dtype;
    return NRLDPC_OK;
}

int nrldpc_last_layers(nrldpc_handle h, int32_t* n_layers) {
    if (!h || !n_layers) return fail(NRLDPC_ERR_ARG, "null handle/out");
    *n_layers = h->last_layers;
    return NRLDPC_OK;
}

int nrldpc_count_layers(int32_t bg, int32_t Z, const void* llr, int32_t batch, int32_t llr_dtype) {
    nrldpc::BaseGraph g;
    if (!nrldpc::base_graph(bg, &g) || nrldpc::set_index(Z) < 0) { (void)fail(NRLDPC_ERR_UNSUPPORTED, "invalid BG / lifting size"); return -1; }
    if (batch < 0 || (batch > 0 && !llr) || llr_dtype < NRLDPC_LLR_F32 || llr_dtype > NRLDPC_LLR_F64) { (void)fail(NRLDPC_ERR_ARG, "invalid llr / batch / llr_dtype"); return -1; }
    const int kind = llr_dtype == NRLDPC_LLR_F64 ? NRLDPC_HQ_F64 : llr_dtype == NRLDPC_LLR_F16 ? NRLDPC_HQ_F16 : NRLDPC_HQ_F32;
    int best = g.kb + 3;
    nrldpc_top_block(llr, kind, (size_t)batch, 0, 1, Z, g.ncols, g.kb + 4, &best);
    return std::max(4, best - g.kb + 1);
}

int nrldpc_set_timing(nrldpc_handle h, int32_t enabled) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    h->timing = enabled != 0;
    h->have_time = false;
    return NRLDPC_OK;
}

int nrldpc_last_kernel_ms(nrldpc_handle h, float* ms) {
    if (!h || !ms) return fail(NRLDPC_ERR_ARG, "null handle/out");
    if (!h->timing || !h->have_time) return fail(NRLDPC_ERR_ARG, "no timed launch recorded");
    HIP_TRY(hipEventSynchronize(h->ev1));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return NRLDPC_OK;
}

int nrldpc_last_host_phases(nrldpc_handle h, double* out10) {
    if (!h || !out10) return fail(NRLDPC_ERR_ARG, "null handle/out");
    if (h->host_phases[0] == 0) return fail(NRLDPC_ERR_ARG, "no chunked host-pointer call recorded on this handle");
    for (int i = 0; i < 10; ++i) out10[i] = h->host_phases[i];
    return NRLDPC_OK;
}

int nrldpc_decode_dev(nrldpc_handle h, const void* d_llr, int32_t batch, uint8_t* d_hard, int32_t* d_iters_out,
                      float* d_app_out, void* stream) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    if (batch < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return NRLDPC_OK;
    if (!d_llr || !d_hard) return fail(NRLDPC_ERR_ARG, "null llr/hard pointer");
    if (h->cfg.llr_dtype == NRLDPC_LLR_F64) return fail(NRLDPC_ERR_ARG, "f64 LLRs are accepted by the host entry point only");
    if (d_app_out && h->cfg.early_term == 2) return fail(NRLDPC_ERR_UNSUPPORTED, "soft output is not available with the CRC-aided stop (early_term = 2)");
    DEVICE_SCOPE(h);
    int nl = 0;
    const int rc = resolve_layers_dev(h, d_llr, batch, static_cast<hipStream_t>(stream), &nl);
    if (rc) return rc;
    return decode_launch(h, d_llr, batch, d_hard, d_iters_out, d_app_out, static_cast<hipStream_t>(stream), nl);
}

int nrldpc_decode_cw_dev(nrldpc_handle h, const void* d_llr, int32_t batch, uint8_t* d_hard, int32_t* d_iters_out,
                         const nrldpc_cw_out* d_out, void* stream) {
    NRLDPC_API_BEGIN
    const int rc = check_cw_args(h, d_llr, batch, d_hard, d_out);
    if (rc) return rc;
    if (batch == 0) return NRLDPC_OK;
    if (h->cfg.llr_dtype == NRLDPC_LLR_F64) return fail(NRLDPC_ERR_ARG, "f64 LLRs are accepted by the host entry point only");
    DEVICE_SCOPE(h);
    return decode_cw_launch(h, d_llr, batch, d_hard, d_iters_out, d_out, static_cast<hipStream_t>(stream));
    NRLDPC_API_END
}

int nrldpc_decode_multi_dev(int32_t n, const nrldpc_handle* hs, const void* const* d_llr, const int32_t* batch,
                            uint8_t* const* d_hard, int32_t* const* d_iters, void* stream) {
    NRLDPC_API_BEGIN
    if (n < 0) return fail(NRLDPC_ERR_ARG, "negative configuration count");
    if (n == 0) return NRLDPC_OK;
    if (!hs || !d_llr || !batch || !d_hard) return fail(NRLDPC_ERR_ARG, "null array");
    for (int i = 0; i < n; ++i) {
        if (!hs[i]) return fail(NRLDPC_ERR_ARG, "null handle");
        if (batch[i] < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
        if (batch[i] > 0 && (!d_llr[i] || !d_hard[i])) return fail(NRLDPC_ERR_ARG, "null llr/hard pointer");
        if (hs[i]->cfg.llr_dtype == NRLDPC_LLR_F64) return fail(NRLDPC_ERR_ARG, "f64 LLRs are accepted by the host entry point only");
        if (hs[i]->cfg.device_id != hs[0]->cfg.device_id) return fail(NRLDPC_ERR_ARG, "all handles of one call must live on one device");
    }
    nrldpc_codec* own = hs[0]; // its scratch holds the tables
    DEVICE_SCOPE(own);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // A configuration whose (BG, Z) has a compile-time-Z kernel (0.55-0.7x the time per codeword) and at least
    // NRLDPC_MULTI_Z64_MIN_ROWS check rows of work (default 512*384: it fills the chip; measured on BASELINE config 4,
    // whose buckets hold ~80 codewords: own launches from 16*384 / 64*384 / 256*384 rows on take 1.47 / 0.89 / 0.58 ms
    // against 0.57 ms with none) gets a launch of its own on that kernel; everything else shares ONE
    // launch of the run-time-Z kernel per (base graph, LLR type): argument blocks, then the workgroup prefix table.
    // All launches of the call are spread over the caller's stream and three side streams (fork / join with events):
    // a bucket's own launch fills only part of the chip, and the shared launches end in a tail of codewords that
    // never converge.
    static const long env_rows = getenv("NRLDPC_MULTI_Z64_MIN_ROWS") ? atol(getenv("NRLDPC_MULTI_Z64_MIN_ROWS")) : 512L * 384L;
    static const bool one_stream = getenv("NRLDPC_MULTI_ONE_STREAM") != nullptr; // A/B
    // The shared launches: one per (base graph, LLR type, workgroup class).  A launch has ONE workgroup size and ONE dynamic-LDS
    // size, and the run-time-Z body keeps every wave of the workgroup to the end: launched together, a 256-thread configuration
    // (27 KB of LDS, four workgroups per CU by its schedule) would run at the residency of a 512-thread one.  Classes: up to 256
    // threads, up to 512, above.  NRLDPC_MULTI_CLASSES=0: one launch per (base graph, LLR type) as before (A/B).
    static const bool env_classes = !(getenv("NRLDPC_MULTI_CLASSES") && atoi(getenv("NRLDPC_MULTI_CLASSES")) == 0);
    constexpr int kClasses = 6;
    static int edges[kClasses] = {256, 512, 768, 768, 768, 768}; // NRLDPC_MULTI_CLASS_EDGES=a,b,...: ascending thread counts (experiments)
    static const bool edges_read = [] {
        const char* e = getenv("NRLDPC_MULTI_CLASS_EDGES");
        for (int i = 0; e && *e && i < kClasses - 1; ++i) {
            edges[i] = atoi(e);
            for (int j = i + 1; j < kClasses; ++j) edges[j] = 768;
            e = strchr(e, ',');
            if (e) ++e;
        }
        return true;
    }();
    (void)edges_read;
    struct Group { std::vector<nrldpc::DecArgs> args; std::vector<int32_t> start; size_t lds = 0; int grid = 0, threads = 0; };
    Group g[2][2][kClasses];
    std::vector<int> routed, bp;
    // layer count of every configuration: its handle's, or (NRLDPC_LAYERS_AUTO) read off its codewords -- all pre-pass kernels
    // are queued first and the stream is synchronised ONCE for the lot
    std::vector<int> nls((size_t)n, 0);
    {
        bool any_auto = false;
        for (int i = 0; i < n; ++i) {
            if (batch[i] == 0) continue;
            if (hs[i]->layers != NRLDPC_LAYERS_AUTO) { nls[i] = hs[i]->layers; continue; }
            for (int j = 0; j < i; ++j)
                if (hs[j] == hs[i] && batch[j] > 0) return fail(NRLDPC_ERR_ARG, "a handle under NRLDPC_LAYERS_AUTO may appear once per nrldpc_decode_multi_dev call");
            const int rc = auto_layers_enqueue(hs[i], d_llr[i], batch[i], st);
            if (rc) return rc;
            any_auto = true;
        }
        if (any_auto) {
            HIP_TRY(hipStreamSynchronize(st));
            for (int i = 0; i < n; ++i)
                if (batch[i] > 0 && hs[i]->layers == NRLDPC_LAYERS_AUTO) nls[i] = auto_layers_read(hs[i]);
        }
    }
    // (Ordering the shared launches' configurations largest lifting size first -- so that the longest workgroups do not start
    // last -- was measured on BASELINE configs[3]: 0.66 ms against 0.61-0.63 ms in the caller's order, twice; not kept.)
    for (int i = 0; i < n; ++i) {
        if (batch[i] == 0) continue;
        nrldpc_codec* h = hs[i];
        const nrldpc::Schedule& s = h->sched;
        if (h->alg == NRLDPC_ALG_SUM_PRODUCT) { bp.push_back(i); continue; } // its own launch on the caller's stream, after the join
        // (a handle with the CRC-aided stop always gets a launch of its own: the shared kernel is built without it)
        if (h->cfg.early_term == 2 || ((long)batch[i] * s.Z >= env_rows && nrldpc::has_z64_kernel(s.g.bg, s.Z))) { routed.push_back(i); continue; }
        int cls = kClasses - 1;
        if (env_classes)
            for (cls = 0; cls < kClasses - 1 && s.threads > edges[cls]; ++cls) {}
        Group& q = g[s.g.bg - 1][h->cfg.llr_dtype == NRLDPC_LLR_F16 ? 1 : 0][cls];
        q.args.push_back(make_dec_args(h, d_llr[i], batch[i], d_hard[i], d_iters ? d_iters[i] : nullptr, nullptr, nls[i]));
        h->last_layers = nls[i];
        q.start.push_back(q.grid);
        q.grid += (batch[i] + s.ncw - 1) / s.ncw;
        q.lds = std::max(q.lds, s.lds_bytes);
        q.threads = std::max(q.threads, s.threads);
    }
    std::vector<char> host;
    size_t off[2][2][kClasses][2];
    int nlaunch = (int)routed.size();
    for (int b = 0; b < 2; ++b)
        for (int d = 0; d < 2; ++d)
            for (int c = 0; c < kClasses; ++c) {
                Group& q = g[b][d][c];
                if (q.args.empty()) continue;
                ++nlaunch;
                q.start.push_back(q.grid);
                host.resize((host.size() + 15) & ~(size_t)15);
                off[b][d][c][0] = host.size();
                host.insert(host.end(), reinterpret_cast<const char*>(q.args.data()),
                            reinterpret_cast<const char*>(q.args.data() + q.args.size()));
                off[b][d][c][1] = host.size();
                host.insert(host.end(), reinterpret_cast<const char*>(q.start.data()),
                            reinterpret_cast<const char*>(q.start.data() + q.start.size()));
            }
    auto bp_launches = [&]() -> int { // the sum-product handles: nrldpc_decode_dev's launch, on the caller's stream
        for (int i : bp) {
            const int r = decode_launch(hs[i], d_llr[i], batch[i], d_hard[i], d_iters ? d_iters[i] : nullptr, nullptr, st, nls[i]);
            if (r) return r;
        }
        return NRLDPC_OK;
    };
    if (nlaunch == 0) return bp_launches();
    // table slot: reused only after the launches that read it have completed (calls on different streams may overlap)
    nrldpc_codec::MultiSlot& m = own->multi[own->multi_next];
    own->multi_next = (own->multi_next + 1) % nrldpc_codec::kMultiSlots;
    if (!m.done) HIP_TRY(hipEventCreateWithFlags(&m.done, hipEventDisableTiming));
    if (m.used) HIP_TRY(hipEventSynchronize(m.done));
    if (!host.empty()) {
        HIP_TRY(m.pin.reserve(host.size()));
        HIP_TRY(m.dev.reserve(host.size()));
        memcpy(m.pin.p, host.data(), host.size());
        HIP_TRY(hipMemcpyAsync(m.dev.p, m.pin.p, host.size(), hipMemcpyHostToDevice, st));
    }
    const bool fan = nlaunch > 1 && !one_stream;
    static const int env_side = getenv("NRLDPC_MULTI_STREAMS") ? atoi(getenv("NRLDPC_MULTI_STREAMS")) : 5;
    const int nside = std::max(1, std::min({env_side, (int)nrldpc_codec::kSide, nlaunch - 1}));
    if (fan) { // fork: the side streams start after the table copy (and everything the caller queued before it)
        if (!own->ev_fork) HIP_TRY(hipEventCreateWithFlags(&own->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(own->ev_fork, st));
        for (int i = 0; i < nside; ++i) {
            if (!own->side[i]) HIP_TRY(hipStreamCreateWithFlags(&own->side[i], hipStreamNonBlocking));
            if (!own->ev_join[i]) HIP_TRY(hipEventCreateWithFlags(&own->ev_join[i], hipEventDisableTiming));
            HIP_TRY(hipStreamWaitEvent(own->side[i], own->ev_fork, 0));
        }
    }
    int rc = NRLDPC_OK, k = 0;
    auto next_stream = [&]() -> hipStream_t { const int q = k++ % (nside + 1); return (!fan || q == 0) ? st : own->side[q - 1]; };
    // shared launches first (the longest: their tail of never-converging small codewords), then the buckets' own
    // (the largest class first: its workgroups are the longest)
    for (int c = kClasses - 1; c >= 0 && rc == NRLDPC_OK; --c)
        for (int b = 0; b < 2 && rc == NRLDPC_OK; ++b)
            for (int d = 0; d < 2 && rc == NRLDPC_OK; ++d) {
                const Group& q = g[b][d][c];
                if (q.args.empty()) continue;
                hipError_t e = nrldpc::launch_decode_multi_wg(
                    b + 1, d ? NRLDPC_K_F16 : NRLDPC_K_F32, reinterpret_cast<const nrldpc::DecArgs*>(m.dev.p + off[b][d][c][0]),
                    reinterpret_cast<const int32_t*>(m.dev.p + off[b][d][c][1]), (int)q.args.size(), q.grid, q.threads, q.lds, next_stream());
                if (e != hipSuccess) rc = hipfail(e, "multi-configuration decode launch");
            }
    for (size_t r = 0; r < routed.size() && rc == NRLDPC_OK; ++r) {
        const int i = routed[r];
        nrldpc_codec* h = hs[i];
        nrldpc::DecArgs a = make_dec_args(h, d_llr[i], batch[i], d_hard[i], d_iters ? d_iters[i] : nullptr, nullptr, nls[i]);
        h->last_layers = nls[i];
        unsigned wslot = 0;
        a.work = a.early_term ? next_work(h, &wslot) : nullptr;
        hipStream_t ls = next_stream();
        hipError_t e = nrldpc::launch_decode(h->sched.g.bg, a, h->sched.threads, h->sched.lds_bytes, ls);
        if (a.work) (void)hipEventRecord(h->work_done[wslot], ls);
        if (e != hipSuccess) rc = hipfail(e, "decode kernel launch");
    }
    if (fan)
        for (int i = 0; i < nside; ++i) { // join: the caller's stream continues after every side launch
            (void)hipEventRecord(own->ev_join[i], own->side[i]);
            (void)hipStreamWaitEvent(st, own->ev_join[i], 0);
        }
    (void)hipEventRecord(m.done, st); // also on a failed launch: the copy above is in flight
    m.used = true;
    if (rc == NRLDPC_OK) rc = bp_launches();
    return rc;
    NRLDPC_API_END
}

int nrldpc_quantise_llr(int8_t* dst, const void* src, int64_t n, int32_t llr_dtype, int32_t llr_scale) {
    if (n <= 0 || !dst || !src) return 0;
    const int kind = llr_dtype == NRLDPC_LLR_F64 ? NRLDPC_HQ_F64 : llr_dtype == NRLDPC_LLR_F16 ? NRLDPC_HQ_F16 : NRLDPC_HQ_F32;
    return nrldpc_quantise_i8(dst, src, (size_t)n, kind, (float)llr_scale) ? 1 : 0;
}

} // extern "C"

namespace {
// nrldpc_decode / nrldpc_decode_packed: `packed` = the hard decisions leave as one BIT per bit ([batch][ceil(K/8)] bytes, least
// significant bit first) instead of one byte per bit -- packed on the device, so that an eighth of the bytes crosses PCIe and
// goes through the copy into the caller's array
// nl_call > 0: the layer count of this call whatever the handle says (nrldpc_pool_*: found once for the whole batch)
// full_scan: under NRLDPC_LAYERS_AUTO scan the whole batch before the first chunk (the restart of a call whose chunk-by-chunk scan
// met a codeword that reaches higher than the first chunk's did)
int decode_host(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out, float* app_out, bool packed,
                int nl_call = 0, bool full_scan = false) {
    NRLDPC_API_BEGIN
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    if (batch < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return NRLDPC_OK;
    if (!llr || !hard) return fail(NRLDPC_ERR_ARG, "null llr/hard pointer");
    if (app_out && h->cfg.early_term == 2) return fail(NRLDPC_ERR_UNSUPPORTED, "soft output is not available with the CRC-aided stop (early_term = 2)");
    DEVICE_SCOPE(h);
    const nrldpc::Schedule& s = h->sched;
    const size_t ncw = (size_t)s.g.ncols * s.Z, K = (size_t)s.g.kb * s.Z;
    const size_t KO = packed ? (K + 7) / 8 : K; // bytes of one codeword's hard decisions in the caller's array
    const size_t cap = (h->cfg.max_batch > batch) ? (size_t)h->cfg.max_batch : (size_t)batch;
    const bool f64 = h->cfg.llr_dtype == NRLDPC_LLR_F64;
    const size_t eb = llr_elem_bytes(h->cfg.llr_dtype); // on the device (MATLAB doubles are narrowed to f32 on the host)
    HIP_TRY(h->s_llr.reserve(cap * ncw * eb));
    HIP_TRY(h->s_hard.reserve(cap * K));
    if (packed) HIP_TRY(h->s_pk.reserve(cap * KO));
    if (iters_out) HIP_TRY(h->s_iters.reserve(cap));
    if (app_out) HIP_TRY(h->s_app.reserve(cap * ncw));

    // Batches above 8 MB: chunks (NRLDPC_HOST_CHUNK_MB of wire bytes, default 32 / 16 as int8; NRLDPC_HOST_THREADS copy threads,
    // default 16, pinned to the caller's NUMA node unless NRLDPC_HOST_NO_PIN is set; NRLDPC_HOST_PIPELINE=0 disables)
    // flow caller array -> pinned slot (copy threads; quantised to int8 on the way when the kernel reads that) -> H2D ->
    // decode -> D2H -> pinned slot -> caller array through four slots on two alternating streams, so that host copies,
    // both DMA directions and the kernels of neighbouring chunks overlap and the host runs up to three chunks ahead of
    // the device.  Same results as one launch (NRLDPC_HOST_TRACE=1: phase times of each call on stderr).
    const size_t in_bytes = (size_t)batch * ncw * eb;
    static const int env_chunk_mb = getenv("NRLDPC_HOST_CHUNK_MB") ? atoi(getenv("NRLDPC_HOST_CHUNK_MB")) : 32;
    static const int env_threads = getenv("NRLDPC_HOST_THREADS") ? atoi(getenv("NRLDPC_HOST_THREADS")) : 16;
    // The copy threads quantise while they copy (1 byte per LLR on the wire instead of 2 / 4; nrldpc_host_quant.h) and a
    // small kernel expands each chunk to fp16 on the device (nrldpc_expand.hip).  NRLDPC_HOST_I8=0: A/B against the native format.
    // Sum-product (NRLDPC_ALG_SUM_PRODUCT) ingests the caller's values unquantised: never this route.
    const bool i8 = h->alg != NRLDPC_ALG_SUM_PRODUCT && !(getenv("NRLDPC_HOST_I8") && atoi(getenv("NRLDPC_HOST_I8")) == 0);
    const int hq_kind = f64 ? NRLDPC_HQ_F64 : h->cfg.llr_dtype == NRLDPC_LLR_F16 ? NRLDPC_HQ_F16 : NRLDPC_HQ_F32;
    const size_t host_eb = f64 ? 8 : eb; // element size of the caller's array
    static const int env_pipe = getenv("NRLDPC_HOST_PIPELINE") ? atoi(getenv("NRLDPC_HOST_PIPELINE")) : 1;
    int nl = nl_call > 0 ? nl_call : h->layers; // NRLDPC_LAYERS_AUTO is resolved below, from the caller's array
    if (env_pipe && in_bytes >= ((size_t)8 << 20) && !app_out && !h->timing) {
        constexpr int NS = nrldpc_codec::kSlots;
        // chunk: ~NRLDPC_HOST_CHUNK_MB of wire bytes (int8 when the copy threads quantise), at least four chunks per call,
        // and -- where that leaves more than one -- whole rounds of 512 codewords (two per CU of a 256-CU device: a
        // 642-codeword chunk ran as one full round and a quarter-full one)
        const size_t wire_eb = i8 ? 1 : eb;
        const size_t chunk_bytes = std::min<size_t>(((size_t)std::max(1, env_chunk_mb) << 20) / (i8 ? 2 : 1), (size_t)batch * ncw * wire_eb / 4);
        int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, chunk_bytes / (ncw * wire_eb)));
        if (chunk >= 512) chunk -= chunk % 512;
        if (!h->pool) {
            // the caller's own thread works too (enqueues, waits for events): leave it a CPU of the quota
            const int want = h->host_threads_hint > 0 ? h->host_threads_hint : std::max(1, env_threads);
            h->pool = new (std::nothrow) HostPool(std::max(1, std::min(want, usable_cpus() - 1)));
            if (!h->pool) return fail(NRLDPC_ERR_NOMEM, "host thread pool");
        }
        h->pool->follow(llr, (size_t)batch * ncw * host_eb);
        struct Hot { // the copy threads poll between the jobs of this call, and sleep again when it returns (whichever way)
            HostPool* p;
            explicit Hot(HostPool* q) : p(q) { p->set_hot(true); }
            ~Hot() { p->set_hot(false); }
        } hot_guard(h->pool);
        // NRLDPC_LAYERS_AUTO, on the copy threads (the all-zero column blocks are read here, once).  Chunk by chunk: the count is
        // taken from the FIRST chunk, and each later chunk's tail above it is checked right before that chunk is quantised -- the
        // device already works on the earlier chunks meanwhile, where a scan of the whole batch up front was a serial phase as long
        // as the quantisation itself (MATLAB doubles at R = 8/9: 5.4 ms a call against 4.0 ms with every row).  A call is rate-
        // matched alike throughout in practice; if a later chunk does reach higher, the call starts again with a full scan.
        const int scan_first = std::min(batch, chunk);
        const bool lazy_scan = nl == NRLDPC_LAYERS_AUTO && !full_scan && scan_first < batch;
        double t_scan = 0;
        auto now_ms = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        if (nl == NRLDPC_LAYERS_AUTO) {
            const double t0 = now_ms();
            nl = layers_of_block(s, h->pool->top_block(llr, hq_kind, (size_t)(lazy_scan ? scan_first : batch), s.Z, s.g.ncols, s.g.kb + 4));
            t_scan += now_ms() - t0;
        }
        // what no active layer reads (extension columns kb + nl ...) is neither quantised nor sent: a row goes out as its first
        // `act` LLRs (int8 wire format only; the kernels never touch the rest of the row -- stale staging bytes at worst)
        const size_t act = i8 ? std::min(ncw, (size_t)(s.g.kb + nl) * (size_t)s.Z) : ncw;
        for (int i = 0; i < NS; ++i) {
            HIP_TRY(h->pin_in[i].reserve((size_t)chunk * ncw * eb));
            HIP_TRY(h->pin_out[i].reserve((size_t)chunk * K));
            if (iters_out) HIP_TRY(h->pin_it[i].reserve((size_t)chunk * 4));
            if (!h->xdone[i]) HIP_TRY(hipEventCreateWithFlags(&h->xdone[i], hipEventDisableTiming));
        }
        const size_t q_slot = ((size_t)chunk * ncw + 255) & ~(size_t)255; // bytes of one int8 chunk on the device
        if (i8) HIP_TRY(h->s_q.reserve(q_slot * NS));
        for (int i = 0; i < 2; ++i)
            if (!h->xs[i]) HIP_TRY(hipStreamCreateWithFlags(&h->xs[i], hipStreamNonBlocking));
        // Chunk k = codewords [starts[k], starts[k+1]).  The first chunk's copy + H2D is the one stretch of a call in which the
        // device has nothing to do, so a call of several rounds opens with two half chunks (one workgroup per CU each).
        // (NRLDPC_HOST_RAMP=1; off by default: measured +-4 % either way on the fp16 path, within the run-to-run spread)
        static const bool env_ramp = getenv("NRLDPC_HOST_RAMP") && atoi(getenv("NRLDPC_HOST_RAMP")) != 0;
        std::vector<int> starts(1, 0);
        for (int pos = 0, k = 0; pos < batch; ++k) {
            const int want = (env_ramp && k < 2 && chunk >= 512 && batch >= 3 * chunk) ? chunk / 2 : chunk;
            pos += std::min(want, batch - pos);
            starts.push_back(pos);
        }
        const int nchunks = (int)starts.size() - 1;
        // an early error return must not leave copies or kernels of this call in flight on the two streams
        struct Quiesce {
            hipStream_t* xs; bool armed = true;
            ~Quiesce() { if (armed) for (int i = 0; i < 2; ++i) if (xs[i]) (void)hipStreamSynchronize(xs[i]); }
        } quiesce{h->xs};
        static const bool trace = getenv("NRLDPC_HOST_TRACE") != nullptr; // phase times of one call on stderr
        double t_quant = 0, t_wait = 0, t_out = 0, t_enq = 0;
        auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        int drained = 0; // chunks 0 .. drained-1 are back in the caller's arrays
        int cur = -1;    // the chunk whose results are on their way out, and how many of its bytes are (it may go out in pieces:
        size_t cur_done = 0; // by the copy threads while they are idle, by this thread while they quantise the next chunk)
        auto drain_step = [&](size_t budget, bool use_pool) -> int { // up to `budget` bytes of chunk `drained`: pinned slot -> caller array
            const int k = drained, sl = k % NS, c0 = starts[k], n = starts[k + 1] - c0;
            const size_t total = (size_t)n * KO;
            if (cur != k) {
                const double t0 = now();
                HIP_TRY(hipEventSynchronize(h->xdone[sl]));
                t_wait += now() - t0;
                cur = k; cur_done = 0;
            }
            const double t1 = now();
            const size_t len = std::min(budget, total - cur_done);
            uint8_t* dst = hard + (size_t)c0 * KO + cur_done;
            const char* src = h->pin_out[sl].p + cur_done;
            if (use_pool && len >= ((size_t)1 << 20)) h->pool->move(dst, src, len, false); // (bit-packed: an eighth of the bytes, not worth a fan-out)
            else memcpy(dst, src, len);
            cur_done += len;
            if (cur_done == total) {
                if (iters_out) memcpy(iters_out + c0, h->pin_it[sl].p, (size_t)n * 4);
                ++drained;
            }
            t_out += now() - t1;
            return NRLDPC_OK;
        };
        auto ready = [&]() { return drained == cur || hipEventQuery(h->xdone[drained % NS]) == hipSuccess; };
        for (int k = 0; k < nchunks; ++k) {
            const int sl = k % NS, st = k & 1, c0 = starts[k], n = starts[k + 1] - c0;
            // the slot's previous chunk has to be out (that also frees pin_in[sl]); chunks that happen to be finished
            // are taken out now (the copy threads are idle) rather than in one lump at the end
            while (drained <= k - NS || (drained < k && ready())) {
                int rc = drain_step((size_t)-1, true); if (rc) return rc;
            }
            const size_t off = (size_t)c0 * ncw;
            if (lazy_scan && c0 + n > scan_first && nl < s.g.nrows) { // (the part of) this chunk the first scan did not see: anything above the count?
                const double t0 = now_ms();
                const int c1 = std::max(c0, scan_first);
                const int top = h->pool->top_block(static_cast<const char*>(llr) + (size_t)c1 * ncw * host_eb, hq_kind, (size_t)(c0 + n - c1), s.Z,
                                                   s.g.ncols, s.g.kb + nl);
                t_scan += now_ms() - t0;
                if (top >= s.g.kb + nl) { // yes: every chunk already sent was decoded with too few rows -- start again, whole-batch scan first
                    for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamSynchronize(h->xs[i]));
                    quiesce.armed = false;
                    return decode_host(h, llr, batch, hard, iters_out, app_out, packed, nl_call, true);
                }
            }
            char* d_in = h->s_llr.p + off * eb;
            int kind = -1; // the handle's own format
            const double tq0 = now();
            // The first chunk is the one stretch of a call in which the device has nothing to do: it is quantised and sent in four
            // pieces, so that its H2D copy overlaps its own quantisation (later chunks overlap the previous chunk's kernel anyway).
            bool as_i8 = i8;
            if (i8) {
                int8_t* d_q = h->s_q.p + q_slot * sl;
                int8_t* pin = reinterpret_cast<int8_t*>(h->pin_in[sl].p);
                const size_t total = (size_t)n * act; // compact: [n][act]
                const int parts = (k == 0 && total >= ((size_t)1 << 20)) ? 4 : 1;
                bool sent = false;
                for (int pi = 0; pi < parts && as_i8; ++pi) {
                    const size_t lo = (total * pi / parts) & ~(size_t)63, hi = pi + 1 == parts ? total : ((total * (pi + 1) / parts) & ~(size_t)63);
                    h->pool->quantise_rows_start(pin, static_cast<const char*>(llr) + off * host_eb, act, ncw, lo, hi, hq_kind, (float)h->scale);
                    // while the copy threads quantise, this thread takes finished chunks' results out, a piece at a time (round 4
                    // ran the two one after the other; with MATLAB doubles the copy threads are the longest phase of a call)
                    while (!h->pool->done() && drained < k && ready()) {
                        int rc = drain_step((size_t)256 << 10, false);
                        if (rc) { (void)h->pool->quantise_rows_finish(); return rc; }
                    }
                    if (h->pool->quantise_rows_finish()) {
                        as_i8 = false; // a -inf: int8 has no code for it (pieces already sent are simply not used)
                    } else {
                        HIP_TRY(hipMemcpyAsync(d_q + lo, pin + lo, hi - lo, hipMemcpyHostToDevice, h->xs[st]));
                        sent = true;
                    }
                }
                if (as_i8) {
                    kind = NRLDPC_K_F16; // whatever the handle's format: this chunk reaches the decoder as fp16
                    HIP_TRY(nrldpc::launch_expand_i8_rows(d_q, d_in, (size_t)n, act, ncw, 1.0f / (float)h->scale, h->xs[st]));
                } else if (sent) {
                    // the pieces already queued still read this pinned slot, which the fallback below overwrites
                    HIP_TRY(hipStreamSynchronize(h->xs[st]));
                }
            }
            if (!as_i8) { // the handle's own format (NRLDPC_HOST_I8=0, or a chunk that holds a -inf)
                if (f64) h->pool->move(h->pin_in[sl].p, static_cast<const double*>(llr) + off, (size_t)n * ncw, true);
                else h->pool->move(h->pin_in[sl].p, static_cast<const char*>(llr) + off * eb, (size_t)n * ncw * eb, false);
                HIP_TRY(hipMemcpyAsync(d_in, h->pin_in[sl].p, (size_t)n * ncw * eb, hipMemcpyHostToDevice, h->xs[st]));
            }
            const double tq1 = now();
            int rc = decode_launch(h, d_in, n, h->s_hard.p + (size_t)c0 * K, iters_out ? h->s_iters.p + c0 : nullptr, nullptr, h->xs[st], nl, kind);
            if (rc) return rc;
            t_quant += tq1 - tq0; t_enq -= tq1;
            if (packed) {
                HIP_TRY(nrldpc::launch_pack_bits(h->s_hard.p + (size_t)c0 * K, h->s_pk.p + (size_t)c0 * KO, n, (int)K, h->xs[st]));
                HIP_TRY(hipMemcpyAsync(h->pin_out[sl].p, h->s_pk.p + (size_t)c0 * KO, (size_t)n * KO, hipMemcpyDeviceToHost, h->xs[st]));
            } else {
                HIP_TRY(hipMemcpyAsync(h->pin_out[sl].p, h->s_hard.p + (size_t)c0 * K, (size_t)n * K, hipMemcpyDeviceToHost, h->xs[st]));
            }
            if (iters_out) HIP_TRY(hipMemcpyAsync(h->pin_it[sl].p, h->s_iters.p + c0, (size_t)n * 4, hipMemcpyDeviceToHost, h->xs[st]));
            HIP_TRY(hipEventRecord(h->xdone[sl], h->xs[st]));
            t_enq += now();
        }
        while (drained < nchunks) { int rc = drain_step((size_t)-1, true); if (rc) return rc; }
        {
            double* ph = h->host_phases;
            ph[0] = nchunks; ph[1] = chunk; ph[2] = nl; ph[3] = t_scan; ph[4] = t_quant; ph[5] = t_enq; ph[6] = t_wait; ph[7] = t_out;
            ph[8] = h->pool->node_; ph[9] = sched_getcpu();
        }
        if (trace)
            fprintf(stderr, "[nrldpc host path] %d chunks of %d, %d layers (%zu of %zu LLRs per codeword on the wire; scan %.2f ms): copy/quantise in %.2f ms (incl. H2D enqueue), launch+D2H enqueue %.2f, wait for device %.2f, copy out %.2f; copy threads on NUMA node %d (caller on CPU %d)\n",
                    nchunks, chunk, nl, act, ncw, t_scan, t_quant, t_enq, t_wait, t_out, h->pool->node_, sched_getcpu());
        quiesce.armed = false; // every chunk was drained behind its event
        return NRLDPC_OK;
    }

    if (nl == NRLDPC_LAYERS_AUTO) { // a small batch: the caller's thread scans it
        int best = s.g.kb + 3;
        nrldpc_top_block(llr, hq_kind, (size_t)batch, 0, 1, s.Z, s.g.ncols, s.g.kb + 4, &best);
        nl = layers_of_block(s, best);
    }
    // The reference's own call pattern -- one step() = the C code blocks of one transport block (NRLDPCDecoder.m:257-266), i.e. a
    // call of one to a few codewords -- is bound by latency, not by bytes: three hipMemcpyAsync calls on pageable memory (each
    // staged and synchronised inside the runtime) and the kernel launches were 0.09 ms of a 0.12 ms call.  Small calls therefore go
    // ZERO-COPY: the caller's LLRs are narrowed / copied into a pinned buffer that the decoder kernel reads over PCIe in its
    // prologue (hipHostMalloc'd memory is device-accessible at the same address), hard decisions (bit-packed by the pack kernel
    // when asked) and iteration counts are written by the kernels straight into pinned memory, and the call is: one CPU copy in,
    // one or two launches, one stream synchronisation, one CPU copy out.  NRLDPC_HOST_ZEROCOPY_KB: largest input (device format)
    // that goes this way, default 2048; 0 = off (A/B).
    static const size_t zc_max = (size_t)(getenv("NRLDPC_HOST_ZEROCOPY_KB") ? atol(getenv("NRLDPC_HOST_ZEROCOPY_KB")) : 2048) << 10;
    if (!app_out && !h->timing && in_bytes <= zc_max) {
        HIP_TRY(h->pin_in[0].reserve(in_bytes));
        HIP_TRY(h->pin_out[0].reserve((size_t)batch * K)); // one byte per bit from the kernel; bit-packed output is packed here, on the CPU
        if (iters_out) HIP_TRY(h->pin_it[0].reserve((size_t)batch * 4));
        if (!h->xs[0]) HIP_TRY(hipStreamCreateWithFlags(&h->xs[0], hipStreamNonBlocking));
        if (f64) {
            const double* d = static_cast<const double*>(llr);
            float* o = reinterpret_cast<float*>(h->pin_in[0].p);
            for (size_t i = 0; i < (size_t)batch * ncw; ++i) o[i] = (float)d[i];
        } else {
            memcpy(h->pin_in[0].p, llr, in_bytes);
        }
        uint8_t* d_out = reinterpret_cast<uint8_t*>(h->pin_out[0].p);
        int rc = decode_launch(h, h->pin_in[0].p, batch, d_out, iters_out ? reinterpret_cast<int32_t*>(h->pin_it[0].p) : nullptr, nullptr, h->xs[0], nl);
        if (rc) { (void)hipStreamSynchronize(h->xs[0]); return rc; }
        HIP_TRY(hipStreamSynchronize(h->xs[0]));
        if (packed) { // a few kilobytes: packing them here saves the pack kernel's launch (one launch per call instead of two)
            for (size_t b = 0; b < (size_t)batch; ++b) {
                const uint8_t* src = d_out + b * K;
                uint8_t* dst = hard + b * KO;
                size_t k = 0;
                for (; k + 8 <= K; k += 8) {
                    uint64_t x;
                    memcpy(&x, src + k, 8);
                    dst[k >> 3] = (uint8_t)(((x & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
                }
                if (k < K) {
                    unsigned v = 0;
                    for (size_t j = k; j < K; ++j) v |= (unsigned)(src[j] & 1u) << (j - k);
                    dst[k >> 3] = (uint8_t)v;
                }
            }
        } else {
            memcpy(hard, d_out, (size_t)batch * K);
        }
        if (iters_out) memcpy(iters_out, h->pin_it[0].p, (size_t)batch * 4);
        return NRLDPC_OK;
    }
    const void* src = llr;
    if (f64) { // MATLAB doubles: narrow on the host (halves PCIe bytes)
        h->h_narrow.resize((size_t)batch * ncw);
        const double* d = static_cast<const double*>(llr);
        for (size_t i = 0; i < (size_t)batch * ncw; ++i) h->h_narrow[i] = (float)d[i];
        src = h->h_narrow.data();
    }
    HIP_TRY(hipMemcpyAsync(h->s_llr.p, src, (size_t)batch * ncw * eb, hipMemcpyHostToDevice, nullptr));
    // F64 was narrowed to f32 above; the kernel sees f32 in that case.
    int rc = decode_launch(h, h->s_llr.p, batch, h->s_hard.p, iters_out ? h->s_iters.p : nullptr,
                           app_out ? h->s_app.p : nullptr, nullptr, nl);
    if (rc) return rc;
    if (packed) {
        HIP_TRY(nrldpc::launch_pack_bits(h->s_hard.p, h->s_pk.p, batch, (int)K, nullptr));
        HIP_TRY(hipMemcpyAsync(hard, h->s_pk.p, (size_t)batch * KO, hipMemcpyDeviceToHost, nullptr));
    } else {
        HIP_TRY(hipMemcpyAsync(hard, h->s_hard.p, (size_t)batch * K, hipMemcpyDeviceToHost, nullptr));
    }
    if (iters_out) HIP_TRY(hipMemcpyAsync(iters_out, h->s_iters.p, (size_t)batch * 4, hipMemcpyDeviceToHost, nullptr));
    if (app_out) HIP_TRY(hipMemcpyAsync(app_out, h->s_app.p, (size_t)batch * ncw * 4, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NRLDPC_OK;
    NRLDPC_API_END
}
} // namespace

extern "C" {

int nrldpc_decode(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out, float* app_out) {
    return decode_host(h, llr, batch, hard, iters_out, app_out, false);
}

int nrldpc_decode_cw(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out, const nrldpc_cw_out* out) {
    NRLDPC_API_BEGIN
    int rc = check_cw_args(h, llr, batch, hard, out);
    if (rc) return rc;
    if (batch == 0) return NRLDPC_OK;
    DEVICE_SCOPE(h);
    const nrldpc::Schedule& s = h->sched;
    const size_t B = (size_t)batch, N = (size_t)s.g.ncols * s.Z, K = (size_t)s.g.kb * s.Z, cbytes = ((size_t)s.g.nrows * s.Z + 7) / 8;
    const size_t eb = llr_elem_bytes(h->cfg.llr_dtype); // on the device: the caller's format, MATLAB doubles narrowed to f32 here
    HIP_TRY(h->s_llr.reserve(B * N * eb));
    HIP_TRY(h->s_hard.reserve(B * K));
    if (iters_out) HIP_TRY(h->s_iters.reserve(B));
    nrldpc_cw_out d = *out;
    if (out->cw_packed) { HIP_TRY(h->s_cw.reserve(B * ((N + 7) / 8))); d.cw_packed = h->s_cw.p; }
    if (out->unsatisfied) { HIP_TRY(h->s_unsat.reserve(B)); d.unsatisfied = h->s_unsat.p; }
    if (out->checks_packed) { HIP_TRY(h->s_chk.reserve(B * cbytes)); d.checks_packed = h->s_chk.p; }
    const void* src = llr;
    if (h->cfg.llr_dtype == NRLDPC_LLR_F64) {
        h->h_narrow.resize(B * N);
        const double* x = static_cast<const double*>(llr);
        for (size_t i = 0; i < B * N; ++i) h->h_narrow[i] = (float)x[i];
        src = h->h_narrow.data();
    }
    HIP_TRY(hipMemcpyAsync(h->s_llr.p, src, B * N * eb, hipMemcpyHostToDevice, nullptr));
    rc = decode_cw_launch(h, h->s_llr.p, batch, h->s_hard.p, iters_out ? h->s_iters.p : nullptr, &d, nullptr);
    if (rc) { (void)hipStreamSynchronize(nullptr); return rc; }
    HIP_TRY(hipMemcpyAsync(hard, h->s_hard.p, B * K, hipMemcpyDeviceToHost, nullptr));
    if (iters_out) HIP_TRY(hipMemcpyAsync(iters_out, h->s_iters.p, B * 4, hipMemcpyDeviceToHost, nullptr));
    if (out->cw_packed) HIP_TRY(hipMemcpyAsync(out->cw_packed, d.cw_packed, B * ((N + 7) / 8), hipMemcpyDeviceToHost, nullptr));
    if (out->unsatisfied) HIP_TRY(hipMemcpyAsync(out->unsatisfied, d.unsatisfied, B * 4, hipMemcpyDeviceToHost, nullptr));
    if (out->checks_packed) HIP_TRY(hipMemcpyAsync(out->checks_packed, d.checks_packed, B * cbytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NRLDPC_OK;
    NRLDPC_API_END
}

int nrldpc_decode_packed(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard_packed, int32_t* iters_out) {
    return decode_host(h, llr, batch, hard_packed, iters_out, nullptr, true);
}

int nrldpc_decode_packed_layers(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard_packed, int32_t* iters_out,
                                int32_t n_layers) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    const int saved = h->layers; // the handle is driven by one caller thread: the count of this call, then the handle's own again
    int rc = nrldpc_set_layers(h, n_layers);
    if (rc != NRLDPC_OK) return rc;
    rc = decode_host(h, llr, batch, hard_packed, iters_out, nullptr, true);
    h->layers = saved;
    return rc;
}

} // extern "C"

// ---- multi-GPU pool: N handles, N host threads, a queue of chunks ------------------------------------------------
struct nrldpc_pool {
    std::vector<nrldpc_handle> hs;
    std::vector<std::thread> th;
    std::vector<int32_t> split;
    int chunks_per_device = 2;
    size_t ncw = 0, K = 0, eb = 0;
    // one job at a time (the pool, like a handle, is driven by one caller thread)
    std::mutex m;
    std::condition_variable cv, cv_done;
    unsigned gen = 0;
    bool stop = false;
    const char* llr = nullptr; uint8_t* hard = nullptr; int32_t* iters = nullptr;
    int batch = 0, chunk = 0, nchunks = 0, next = 0, running = 0, rc = NRLDPC_OK;
    bool packed = false; // hard decisions leave bit-packed (nrldpc_pool_decode_packed)
    int layers = 0;      // as nrldpc_codec::layers (nrldpc_pool_set_layers); nl_call: what this call runs with
    int nl_call = 0;
    // NRLDPC_LAYERS_AUTO, device form: every shard scans its slice, the last one to arrive takes the maximum, all launch with it
    int scan_arrived = 0, scan_best = 0;
    std::condition_variable cv_scan;
    std::string err;
    // device-resident job (nrldpc_pool_decode_dev): shard i launches on its own stream and waits for it
    bool dev_job = false;
    const void* const* dv_llr = nullptr; const int32_t* dv_batch = nullptr; uint8_t* const* dv_hard = nullptr;
    int32_t* const* dv_iters = nullptr;
    std::vector<hipStream_t> streams;

    int decode_dev_shard(int i) {
        if (dv_batch[i] <= 0) return dv_batch[i] < 0 ? fail(NRLDPC_ERR_ARG, "negative batch") : NRLDPC_OK;
        nrldpc_handle h = hs[i];
        DEVICE_SCOPE(h);
        if (!streams[i]) HIP_TRY(hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking));
        // The shard's stream is private and non-blocking, so it is ordered against nothing the caller queued: wait for
        // everything already submitted to this device (whatever stream produced d_llr[i]) before the launch.  The call is
        // synchronous anyway -- it returns when every shard is done -- so this costs no overlap the caller could have had.
        HIP_TRY(hipDeviceSynchronize());
        if (h->cfg.llr_dtype == NRLDPC_LLR_F64) return fail(NRLDPC_ERR_ARG, "f64 LLRs are accepted by the host entry point only");
        const int r = decode_launch(h, dv_llr[i], dv_batch[i], dv_hard[i], dv_iters ? dv_iters[i] : nullptr, nullptr, streams[i], nl_call);
        if (r != NRLDPC_OK) return r;
        HIP_TRY(hipStreamSynchronize(streams[i]));
        return NRLDPC_OK;
    }
    // first phase of a device-form call under NRLDPC_LAYERS_AUTO: this shard's highest non-zero column block (first - 1: none)
    int scan_dev_shard(int i, int* top) {
        nrldpc_handle h = hs[i];
        *top = h->sched.g.kb + 3;
        if (dv_batch[i] <= 0 || h->cfg.llr_dtype == NRLDPC_LLR_F64) return NRLDPC_OK; // (errors are reported by the decode phase)
        DEVICE_SCOPE(h);
        if (!streams[i]) HIP_TRY(hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking));
        HIP_TRY(hipDeviceSynchronize());
        const int r = auto_layers_enqueue(h, dv_llr[i], dv_batch[i], streams[i]);
        if (r != NRLDPC_OK) return r;
        HIP_TRY(hipStreamSynchronize(streams[i]));
        *top = *reinterpret_cast<const int32_t*>(h->pin_best.p);
        return NRLDPC_OK;
    }

    void worker(int i) {
        unsigned seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
            }
            if (dev_job) {
                if (layers == NRLDPC_LAYERS_AUTO) {
                    int top = 0;
                    const int rs = scan_dev_shard(i, &top);
                    std::unique_lock<std::mutex> lk(m);
                    if (rs != NRLDPC_OK && rc == NRLDPC_OK) { rc = rs; err = nrldpc_last_error(); }
                    scan_best = std::max(scan_best, top);
                    if (++scan_arrived == (int)hs.size()) {
                        nl_call = layers_of_block(hs[0]->sched, scan_best);
                        cv_scan.notify_all();
                    } else {
                        cv_scan.wait(lk, [&] { return scan_arrived == (int)hs.size(); });
                    }
                    if (rc != NRLDPC_OK) { // some shard's scan failed: nobody launches
                        split[i] = 0;
                        if (--running == 0) cv_done.notify_all();
                        continue;
                    }
                }
                const int r = decode_dev_shard(i);
                std::lock_guard<std::mutex> lk(m);
                if (r != NRLDPC_OK && rc == NRLDPC_OK) { rc = r; err = nrldpc_last_error(); }
                split[i] = dv_batch[i] > 0 ? dv_batch[i] : 0;
            } else for (;;) {
                int k;
                {
                    std::lock_guard<std::mutex> lk(m);
                    if (next >= nchunks || rc != NRLDPC_OK) break;
                    k = next++;
                }
                const int c0 = k * chunk, n = std::min(chunk, batch - c0);
                const int r = decode_host(hs[i], llr + (size_t)c0 * ncw * eb, n, hard + (size_t)c0 * (packed ? (K + 7) / 8 : K),
                                          iters ? iters + c0 : nullptr, nullptr, packed, nl_call);
                std::lock_guard<std::mutex> lk(m);
                if (r != NRLDPC_OK && rc == NRLDPC_OK) { rc = r; err = nrldpc_last_error(); }
                split[i] += n;
            }
            std::lock_guard<std::mutex> lk(m);
            if (--running == 0) cv_done.notify_all();
        }
    }
};

extern "C" {

int nrldpc_pool_create(const nrldpc_cfg* cfg, const int32_t* device_ids, int32_t n_devices, int32_t chunks_per_device,
                       nrldpc_pool_handle* out) {
    NRLDPC_API_BEGIN
    if (!cfg || !device_ids || !out) return fail(NRLDPC_ERR_ARG, "null cfg/device_ids/out");
    *out = nullptr;
    // before anything reads *cfg as this library's struct: a caller built against another revision may have passed a smaller one
    if (cfg->struct_size != (uint32_t)sizeof(nrldpc_cfg))
        return fail(NRLDPC_ERR_ARG, "nrldpc_cfg.struct_size does not match this library (set it to sizeof(nrldpc_cfg); ABI revision mismatch?)");
    if (n_devices < 1 || n_devices > 64) return fail(NRLDPC_ERR_ARG, "n_devices must be in 1..64");
    if (chunks_per_device < 1 || chunks_per_device > 64) return fail(NRLDPC_ERR_ARG, "chunks_per_device must be in 1..64");
    nrldpc_pool* p = new nrldpc_pool();
    p->chunks_per_device = chunks_per_device;
    for (int i = 0; i < n_devices; ++i) {
        nrldpc_cfg c = *cfg;
        c.device_id = device_ids[i];
        nrldpc_handle h = nullptr;
        const int rc = nrldpc_create(&c, &h);
        if (rc != NRLDPC_OK) {
            for (auto q : p->hs) nrldpc_destroy(q);
            delete p;
            return rc; // text of nrldpc_create's failure is already in place
        }
        h->host_threads_hint = std::max(2, 16 / n_devices);
        p->hs.push_back(h);
    }
    const nrldpc::Schedule& s = p->hs[0]->sched;
    p->ncw = (size_t)s.g.ncols * s.Z; p->K = (size_t)s.g.kb * s.Z;
    p->eb = cfg->llr_dtype == NRLDPC_LLR_F64 ? 8 : cfg->llr_dtype == NRLDPC_LLR_F16 ? 2 : 4; // in the caller's array
    p->layers = p->hs[0]->layers;
    p->split.assign(n_devices, 0);
    p->streams.assign(n_devices, nullptr);
    for (int i = 0; i < n_devices; ++i) p->th.emplace_back([p, i] { p->worker(i); });
    *out = p;
    return NRLDPC_OK;
    NRLDPC_API_END
}

} // extern "C"
namespace {
int pool_decode_host(nrldpc_pool_handle p, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out, bool packed) {
    NRLDPC_API_BEGIN
    if (!p) return fail(NRLDPC_ERR_ARG, "null pool");
    if (batch < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return NRLDPC_OK;
    if (!llr || !hard) return fail(NRLDPC_ERR_ARG, "null llr/hard pointer");
    std::unique_lock<std::mutex> lk(p->m);
    p->packed = packed;
    p->nl_call = p->layers;
    if (p->layers == NRLDPC_LAYERS_AUTO) { // once for the whole batch, before it is cut: a few short-lived threads over the caller's array
        const nrldpc::Schedule& s = p->hs[0]->sched;
        const int kind = p->eb == 8 ? NRLDPC_HQ_F64 : p->eb == 2 ? NRLDPC_HQ_F16 : NRLDPC_HQ_F32;
        const int nt = std::max(1, std::min({8, usable_cpus(), batch}));
        int best = s.g.kb + 3;
        std::vector<std::thread> ts;
        for (int t = 1; t < nt; ++t)
            ts.emplace_back([&, t] { nrldpc_top_block(llr, kind, (size_t)batch, (size_t)t, (size_t)nt, s.Z, s.g.ncols, s.g.kb + 4, &best); });
        nrldpc_top_block(llr, kind, (size_t)batch, 0, (size_t)nt, s.Z, s.g.ncols, s.g.kb + 4, &best);
        for (auto& t : ts) t.join();
        p->nl_call = layers_of_block(s, best);
    }
    const int want = (int)p->hs.size() * p->chunks_per_device;
    p->chunk = std::max(1, (batch + want - 1) / want);
    p->nchunks = (batch + p->chunk - 1) / p->chunk;
    p->llr = static_cast<const char*>(llr); p->hard = hard; p->iters = iters_out; p->batch = batch;
    p->next = 0; p->rc = NRLDPC_OK; p->err.clear();
    p->dev_job = false;
    std::fill(p->split.begin(), p->split.end(), 0);
    p->running = (int)p->th.size();
    ++p->gen;
    p->cv.notify_all();
    p->cv_done.wait(lk, [&] { return p->running == 0; });
    if (p->rc != NRLDPC_OK) return fail(p->rc, p->err);
    return NRLDPC_OK;
    NRLDPC_API_END
}
} // namespace
extern "C" {

int nrldpc_pool_decode(nrldpc_pool_handle p, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out) {
    return pool_decode_host(p, llr, batch, hard, iters_out, false);
}
int nrldpc_pool_decode_packed(nrldpc_pool_handle p, const void* llr, int32_t batch, uint8_t* hard_packed, int32_t* iters_out) {
    return pool_decode_host(p, llr, batch, hard_packed, iters_out, true);
}

int nrldpc_pool_set_layers(nrldpc_pool_handle p, int32_t n_layers) {
    if (!p) return fail(NRLDPC_ERR_ARG, "null pool");
    std::lock_guard<std::mutex> lk(p->m);
    for (auto h : p->hs) {
        const int rc = nrldpc_set_layers(h, n_layers);
        if (rc != NRLDPC_OK) return rc;
    }
    p->layers = p->hs[0]->layers;
    return NRLDPC_OK;
}

int nrldpc_pool_set_algorithm(nrldpc_pool_handle p, int32_t algorithm) {
    if (!p) return fail(NRLDPC_ERR_ARG, "null pool");
    std::lock_guard<std::mutex> lk(p->m);
    for (auto h : p->hs) { // the shards share one nrldpc_cfg: the first refusal comes before any shard changed
        const int rc = nrldpc_set_algorithm(h, algorithm);
        if (rc != NRLDPC_OK) return rc;
    }
    return NRLDPC_OK;
}

int nrldpc_pool_decode_dev(nrldpc_pool_handle p, const void* const* d_llr, const int32_t* batch, uint8_t* const* d_hard,
                           int32_t* const* d_iters) {
    NRLDPC_API_BEGIN
    if (!p) return fail(NRLDPC_ERR_ARG, "null pool");
    if (!d_llr || !batch || !d_hard) return fail(NRLDPC_ERR_ARG, "null d_llr/batch/d_hard array");
    for (size_t i = 0; i < p->hs.size(); ++i)
        if (batch[i] > 0 && (!d_llr[i] || !d_hard[i])) return fail(NRLDPC_ERR_ARG, "null device pointer for a shard with work");
    std::unique_lock<std::mutex> lk(p->m);
    p->dev_job = true;
    p->nl_call = p->layers; p->scan_arrived = 0; p->scan_best = 0;
    p->dv_llr = d_llr; p->dv_batch = batch; p->dv_hard = d_hard; p->dv_iters = d_iters;
    p->rc = NRLDPC_OK; p->err.clear();
    std::fill(p->split.begin(), p->split.end(), 0);
    p->running = (int)p->th.size();
    ++p->gen;
    p->cv.notify_all();
    p->cv_done.wait(lk, [&] { return p->running == 0; });
    p->dev_job = false;
    if (p->rc != NRLDPC_OK) return fail(p->rc, p->err);
    return NRLDPC_OK;
    NRLDPC_API_END
}

int nrldpc_pool_set_timing(nrldpc_pool_handle p, int32_t enabled) {
    if (!p) return fail(NRLDPC_ERR_ARG, "null pool");
    std::lock_guard<std::mutex> lk(p->m);
    for (auto h : p->hs) {
        const int rc = nrldpc_set_timing(h, enabled);
        if (rc != NRLDPC_OK) return rc;
    }
    return NRLDPC_OK;
}

int nrldpc_pool_last_kernel_ms(nrldpc_pool_handle p, float* ms) {
    NRLDPC_API_BEGIN
    if (!p || !ms) return fail(NRLDPC_ERR_ARG, "null pool/out");
    std::lock_guard<std::mutex> lk(p->m);
    for (size_t i = 0; i < p->hs.size(); ++i) {
        nrldpc_handle h = p->hs[i];
        ms[i] = 0.0f;
        if (!h->timing) return fail(NRLDPC_ERR_ARG, "timing is not enabled (nrldpc_pool_set_timing)");
        if (!h->have_time) continue; // this shard has not launched since timing was enabled
        DEVICE_SCOPE(h);
        HIP_TRY(hipEventSynchronize(h->ev1));
        HIP_TRY(hipEventElapsedTime(&ms[i], h->ev0, h->ev1));
    }
    return NRLDPC_OK;
    NRLDPC_API_END
}

int nrldpc_pool_size(nrldpc_pool_handle p) { return p ? (int)p->hs.size() : 0; }

int nrldpc_pool_last_split(nrldpc_pool_handle p, int32_t* counts) {
    if (!p || !counts) return fail(NRLDPC_ERR_ARG, "null pool/counts");
    std::lock_guard<std::mutex> lk(p->m);
    for (size_t i = 0; i < p->split.size(); ++i) counts[i] = p->split[i];
    return NRLDPC_OK;
}

void nrldpc_pool_destroy(nrldpc_pool_handle p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(p->m);
        p->stop = true;
    }
    p->cv.notify_all();
    for (auto& t : p->th) t.join();
    for (size_t i = 0; i < p->hs.size(); ++i)
        if (p->streams[i]) { DeviceScope scope(p->hs[i]->cfg.device_id); (void)hipStreamDestroy(p->streams[i]); }
    for (auto h : p->hs) nrldpc_destroy(h);
    delete p;
}

static uint32_t crc_poly_for(int len, bool code_block) {
    // get_3gpp_crc_polynomial.m:3-14
    if (len == 16) return 0x11021u;
    return code_block ? 0x1800063u : 0x1864CFBu;
}

// x^n mod g as an L-bit register value
static uint32_t xpow_mod(uint32_t poly, int L, long n) {
    const uint32_t top = 1u << (L - 1), mask = (1u << L) - 1u;
    uint32_t v = 1u; // x^0
    for (long i = 0; i < n; ++i) {
        const bool carry = v & top;
        v = (v << 1) & mask;
        if (carry) v ^= poly & mask;
    }
    return v;
}

static void xpow_matrix(uint32_t* M, uint32_t poly, int L, long n) {
    const uint32_t top = 1u << (L - 1), mask = (1u << L) - 1u;
    uint32_t v = xpow_mod(poly, L, n); // x^n
    for (int b = 0; b < 24; ++b) {
        M[b] = (b < L) ? v : 0u; // x^(n+b)
        const bool carry = v & top;
        v = (v << 1) & mask;
        if (carry) v ^= poly & mask;
    }
}

// Plan for wave-parallel CRCs over messages of up to `len` bits; seg / seg_tail are the segment lengths of
// the cross-code-block fold (nrldpc_crc.hip).  An odd chunk keeps the 64 lanes' LDS reads on distinct banks.
static void make_crc_plan(nrldpc::CrcPlan* pl, uint32_t poly, int L, int len, int seg, int seg_tail) {
    pl->poly = poly; pl->L = L;
    pl->chunk = ((len + 63) / 64) | 1;
    for (int s = 0; s < 6; ++s) xpow_matrix(pl->shiftmat[s], poly, L, (long)pl->chunk << s);
    xpow_matrix(pl->horner, poly, L, seg);
    xpow_matrix(pl->horner_tail, poly, L, seg_tail);
}

static int check_tb_params(const nrldpc_tb_params* p) {
    if (!p) return fail(NRLDPC_ERR_ARG, "null parameters");
    if (p->C < 1 || p->C > NRLDPC_MAX_C) return fail(NRLDPC_ERR_UNSUPPORTED, "C out of range (1..160)");
    if (nrldpc::set_index(p->Z) < 0 || (p->bg != 1 && p->bg != 2)) return fail(NRLDPC_ERR_UNSUPPORTED, "invalid BG / lifting size");
    if (p->Q_m < 1 || p->N_cb < 1 || p->N_cb > p->N || p->K_prime > p->K) return fail(NRLDPC_ERR_UNSUPPORTED, "inconsistent block parameters");
    return NRLDPC_OK;
}

static int make_rm_args(const nrldpc_tb_params* p, const float* d_g_tilde, int32_t n_tb, float* d_harq, void* d_cw_llr,
                        int32_t out_dtype, nrldpc::RmArgs* out) {
    // G == 0 is a legal draw of the reference's own sweep (testbench.m:35 with a small A): nothing was transmitted, the
    // decoder input is all zeros / fillers, and an empty g_tilde has no address
    if (!d_g_tilde && p->G > 0) return fail(NRLDPC_ERR_ARG, "null pointer");
    nrldpc::RmArgs& a = *out;
    memset(&a, 0, sizeof a);
    a.g = d_g_tilde; a.harq = d_harq; a.out = d_cw_llr; a.out_f16 = out_dtype == NRLDPC_LLR_F16;
    return fill_rm_blocks(p, n_tb, a);
}

int nrldpc_rate_recover_dev(const nrldpc_tb_params* p, const float* d_g_tilde, int32_t n_tb, float* d_harq,
                            void* d_cw_llr, int32_t out_dtype, void* stream) {
    int rc = check_tb_params(p);
    if (rc) return rc;
    if (n_tb < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (n_tb == 0) return NRLDPC_OK;
    if (!d_cw_llr) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (out_dtype != NRLDPC_LLR_F32 && out_dtype != NRLDPC_LLR_F16) return fail(NRLDPC_ERR_ARG, "out_dtype must be f32 or f16");
    nrldpc::RmArgs a;
    rc = make_rm_args(p, d_g_tilde, n_tb, d_harq, d_cw_llr, out_dtype, &a);
    if (rc) return rc;
    hipError_t e = nrldpc::launch_rate_recover(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "rate-recovery kernel launch");
    return NRLDPC_OK;
}

int nrldpc_rate_recover_ex_dev(const nrldpc_tb_params* p, const void* d_g_tilde, int32_t in_dtype, int32_t n_tb,
                               void* d_harq, int32_t harq_dtype, void* d_cw_llr, int32_t out_dtype, void* stream) {
    static_assert(nrldpc::RMX_MAX_C == NRLDPC_MAX_C, "RmExArgs holds one entry per code block");
    int rc = check_tb_params(p);
    if (rc) return rc;
    auto known = [](int32_t d) { return d == NRLDPC_LLR_F32 || d == NRLDPC_LLR_F16; };
    if (!known(in_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "in_dtype must be f32 or f16");
    if (d_harq && !known(harq_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "harq_dtype must be f32 or f16");
    if (!known(out_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "out_dtype must be f32 or f16");
    if (n_tb < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (n_tb == 0) return NRLDPC_OK;
    if (!d_cw_llr || (!d_g_tilde && p->G > 0)) return fail(NRLDPC_ERR_ARG, "null pointer");
    nrldpc::RmExArgs a;
    memset(&a, 0, sizeof a);
    a.g = d_g_tilde; a.harq = d_harq; a.out = d_cw_llr;
    a.in_f16 = in_dtype == NRLDPC_LLR_F16; a.harq_f16 = d_harq && harq_dtype == NRLDPC_LLR_F16; a.out_f16 = out_dtype == NRLDPC_LLR_F16;
    rc = fill_rm_blocks(p, n_tb, a);
    if (rc) return rc;
    hipError_t e = nrldpc::launch_rate_recover_ex(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "rate-recovery kernel launch");
    return NRLDPC_OK;
}

static int crc_check_common(const nrldpc_tb_params* p, const uint8_t* d_c_hat, int32_t n_tb, uint8_t* d_b_hat, int32_t* d_ok,
                            int32_t* d_cb_pass, const uint8_t* cbgti_flags, int keep_b_hat, int sticky, void* stream) {
    int rc = check_tb_params(p);
    if (rc) return rc;
    if (n_tb < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (n_tb == 0) return NRLDPC_OK;
    if (!d_c_hat || !d_b_hat || !d_ok) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (sticky && !d_cb_pass) return fail(NRLDPC_ERR_ARG, "the sticky code-block flags (d_cb_pass) are required");
    if ((p->tb_crc_len != 16 && p->tb_crc_len != 24) || (p->cb_crc_len != 0 && p->cb_crc_len != 24))
        return fail(NRLDPC_ERR_UNSUPPORTED, "CRC lengths must be 16/24 (TB) and 0/24 (CB)");
    if (p->B != p->A + p->tb_crc_len || p->C * (p->K_prime - p->cb_crc_len) != p->B)
        return fail(NRLDPC_ERR_ARG, "B must equal A + L and C*(K' - L_cb)");
    nrldpc::CrcArgs a;
    a.c_hat = d_c_hat; a.b_hat = d_b_hat; a.ok = d_ok; a.cb_pass = d_cb_pass;
    a.n_tb = n_tb; a.C = p->C; a.K = p->K; a.Kp = p->K_prime; a.Lcb = p->cb_crc_len; a.A = p->A; a.B = p->B;
    a.keep_b_hat = keep_b_hat ? 1 : 0; a.sticky = sticky ? 1 : 0;
    for (int r = 0; r < NRLDPC_MAX_C; ++r) a.cbgti[r] = (cbgti_flags && r < p->C) ? (cbgti_flags[r] ? 1 : 0) : 1;
    const int pay = p->K_prime - p->cb_crc_len;
    make_crc_plan(&a.tb, crc_poly_for(p->tb_crc_len, false), p->tb_crc_len, pay, pay, pay);
    make_crc_plan(&a.cb, crc_poly_for(24, true), 24, p->K_prime, 0, 0);
    hipError_t e = nrldpc::launch_crc_check(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "CRC kernel launch");
    return NRLDPC_OK;
}

int nrldpc_crc_check_dev(const nrldpc_tb_params* p, const uint8_t* d_c_hat, int32_t n_tb, uint8_t* d_b_hat,
                         int32_t* d_ok, int32_t* d_cb_pass, void* stream) {
    return crc_check_common(p, d_c_hat, n_tb, d_b_hat, d_ok, d_cb_pass, nullptr, 0, 0, stream);
}

int nrldpc_crc_check_harq_dev(const nrldpc_tb_params* p, const uint8_t* d_c_hat, int32_t n_tb, uint8_t* d_b_hat,
                              int32_t* d_ok, int32_t* d_cb_pass, const uint8_t* cbgti_flags, int32_t keep_b_hat,
                              void* stream) {
    return crc_check_common(p, d_c_hat, n_tb, d_b_hat, d_ok, d_cb_pass, cbgti_flags, keep_b_hat, 1, stream);
}

int nrldpc_crc_attach_dev(const nrldpc_tb_params* p, const uint8_t* d_a, int32_t n_tb, uint8_t* d_c, void* stream) {
    int rc = check_tb_params(p);
    if (rc) return rc;
    if (n_tb < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (n_tb == 0) return NRLDPC_OK;
    if (!d_a || !d_c) return fail(NRLDPC_ERR_ARG, "null pointer");
    if ((p->tb_crc_len != 16 && p->tb_crc_len != 24) || (p->cb_crc_len != 0 && p->cb_crc_len != 24))
        return fail(NRLDPC_ERR_UNSUPPORTED, "CRC lengths must be 16/24 (TB) and 0/24 (CB)");
    if (p->B != p->A + p->tb_crc_len || p->C * (p->K_prime - p->cb_crc_len) != p->B)
        return fail(NRLDPC_ERR_ARG, "B must equal A + L and C*(K' - L_cb)");
    nrldpc::CrcAttachArgs a;
    a.a = d_a; a.c = d_c; a.n_tb = n_tb; a.C = p->C; a.K = p->K; a.Kp = p->K_prime; a.Lcb = p->cb_crc_len;
    a.A = p->A; a.B = p->B;
    const int pay = p->K_prime - p->cb_crc_len;
    if (pay < p->tb_crc_len) return fail(NRLDPC_ERR_UNSUPPORTED, "code block shorter than the transport-block CRC");
    make_crc_plan(&a.tb, crc_poly_for(p->tb_crc_len, false), p->tb_crc_len, pay, pay, pay - p->tb_crc_len);
    make_crc_plan(&a.cb, crc_poly_for(24, true), 24, pay, 0, 0);
    hipError_t e = nrldpc::launch_crc_attach(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "CRC attach kernel launch");
    return NRLDPC_OK;
}

int nrldpc_rate_match_dev(const nrldpc_tb_params* p, const uint8_t* d_cw, int32_t n_tb, uint8_t* d_g, void* stream) {
    int rc = check_tb_params(p);
    if (rc) return rc;
    if (n_tb < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (n_tb == 0) return NRLDPC_OK;
    if (p->G == 0) return NRLDPC_OK; // nothing to transmit (testbench.m:35 can draw G = 0); g has no address then
    if (!d_cw || !d_g) return fail(NRLDPC_ERR_ARG, "null pointer");
    nrldpc::TxRmArgs a;
    a.cw = d_cw; a.g = d_g; a.n_tb = n_tb; a.C = p->C; a.G = p->G; a.Z = p->Z; a.K = p->K; a.Kp = p->K_prime;
    a.N = p->N; a.N_cb = p->N_cb; a.k0 = p->k_0; a.Qm = p->Q_m;
    int off = 0;
    for (int r = 0; r < p->C; ++r) {
        if (p->E_r[r] < 0 || p->E_r[r] % p->Q_m) return fail(NRLDPC_ERR_UNSUPPORTED, "E_r must be a non-negative multiple of Q_m");
        a.E[r] = p->E_r[r]; a.off[r] = off; off += p->E_r[r];
    }
    if (off != p->G) return fail(NRLDPC_ERR_ARG, "sum(E_r) must equal G");
    hipError_t e = nrldpc::launch_rate_match(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "rate-matching kernel launch");
    return NRLDPC_OK;
}

int nrldpc_awgn_llr_dev(const uint8_t* d_g, int64_t n_bits, int32_t Q_m, float EsN0_dB, uint64_t seed,
                        uint64_t first_symbol, float* d_g_tilde, void* stream) {
    if (Q_m != 1 && Q_m != 2 && Q_m != 4 && Q_m != 6 && Q_m != 8) return fail(NRLDPC_ERR_UNSUPPORTED, "Unsupported modulation");
    if (n_bits < 0 || n_bits % Q_m) return fail(NRLDPC_ERR_ARG, "n_bits must be a non-negative multiple of Q_m");
    if (n_bits == 0) return NRLDPC_OK;
    if (!d_g || !d_g_tilde) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (!(EsN0_dB > -60.0f && EsN0_dB < 80.0f)) return fail(NRLDPC_ERR_ARG, "EsN0_dB out of range");
    nrldpc::ChanArgs a;
    a.g = d_g; a.llr = d_g_tilde; a.n_sym = n_bits / Q_m; a.seed = seed; a.first_symbol = first_symbol; a.Qm = Q_m;
    const double n0 = std::pow(10.0, -(double)EsN0_dB / 10.0); // plot_BLER_vs_SNR.m:106
    static const double mean_sq[5] = {1.0, 1.0, 5.0, 21.0, 85.0};  // mean(level^2) of a rail with 0,1,2,3,4 bits
    a.sigma = (float)std::sqrt(n0 / 2.0); a.inv_n0 = (float)(1.0 / n0);
    a.inv_norm = (float)(1.0 / std::sqrt(2.0 * mean_sq[Q_m / 2]));
    hipError_t e = nrldpc::launch_awgn_llr(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "channel kernel launch");
    return NRLDPC_OK;
}

// ---- stand-alone mapper / demapper (nrldpc_modem.hip): every check before any device call ----
static const double kRailMeanSq[5] = {1.0, 1.0, 5.0, 21.0, 85.0}; // mean(level^2) of a rail with 0,1,2,3,4 bits

int nrldpc_modulate_dev(const uint8_t* d_g, int64_t n_bits, int32_t Q_m, float* d_tx, void* stream) {
    if (Q_m != 1 && Q_m != 2 && Q_m != 4 && Q_m != 6 && Q_m != 8) return fail(NRLDPC_ERR_UNSUPPORTED, "Unsupported modulation");
    if (n_bits < 0 || n_bits % Q_m) return fail(NRLDPC_ERR_ARG, "n_bits must be a non-negative multiple of Q_m");
    if (n_bits == 0) return NRLDPC_OK;
    if (!d_g || !d_tx) return fail(NRLDPC_ERR_ARG, "null pointer");
    nrldpc::ModArgs a;
    a.g = d_g; a.tx = d_tx; a.n_sym = n_bits / Q_m; a.Qm = Q_m;
    a.inv_norm = (float)(1.0 / std::sqrt(2.0 * kRailMeanSq[Q_m / 2]));
    hipError_t e = nrldpc::launch_modulate(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mapper kernel launch");
    return NRLDPC_OK;
}

int nrldpc_demodulate_dev(const float* d_rx, int64_t n_sym, int32_t Q_m, int32_t method, float variance, const float* d_variance,
                          void* d_out, int32_t out_dtype, void* stream) {
    if (Q_m != 1 && Q_m != 2 && Q_m != 4 && Q_m != 6 && Q_m != 8) return fail(NRLDPC_ERR_UNSUPPORTED, "Unsupported modulation");
    if (method != NRLDPC_DEMOD_LLR && method != NRLDPC_DEMOD_APPROX_LLR && method != NRLDPC_DEMOD_HARD)
        return fail(NRLDPC_ERR_UNSUPPORTED, "unknown decision method");
    const bool hard = method == NRLDPC_DEMOD_HARD;
    if (!hard && out_dtype != NRLDPC_LLR_F32 && out_dtype != NRLDPC_LLR_F16) return fail(NRLDPC_ERR_UNSUPPORTED, "out_dtype must be f32 or f16");
    if (n_sym < 0) return fail(NRLDPC_ERR_ARG, "negative symbol count");
    if (n_sym > 0 && (!d_rx || !d_out)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (!d_variance && !(variance > 0.0f && std::isfinite(variance))) return fail(NRLDPC_ERR_ARG, "variance must be positive and finite");
    if (n_sym == 0) return NRLDPC_OK;
    nrldpc::DemodArgs a;
    a.rx = d_rx; a.var = d_variance; a.out = d_out; a.n_sym = n_sym; a.Qm = Q_m; a.method = method; a.out_dtype = out_dtype;
    a.variance = d_variance ? 1.0f : variance;
    a.inv_norm = (float)(1.0 / std::sqrt(2.0 * kRailMeanSq[Q_m / 2]));
    hipError_t e = nrldpc::launch_demodulate(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "demapper kernel launch");
    return NRLDPC_OK;
}

// ---- stand-alone AWGN stage (nrldpc_awgn.hip): every check before any device call ----
int nrldpc_awgn_dev(const float* d_tx, int64_t n_sym, float variance, const float* d_variance, uint64_t seed, uint64_t first_symbol,
                    float* d_rx, void* stream) {
    if (n_sym < 0) return fail(NRLDPC_ERR_ARG, "negative symbol count");
    if (n_sym > 0 && (!d_tx || !d_rx)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (!d_variance && !(variance >= 0.0f && std::isfinite(variance))) return fail(NRLDPC_ERR_ARG, "variance must be non-negative and finite");
    if (first_symbol + (uint64_t)n_sym < first_symbol) return fail(NRLDPC_ERR_ARG, "first_symbol + n_sym overflows 64 bits");
    if (n_sym == 0) return NRLDPC_OK;
    nrldpc::AwgnArgs a;
    a.tx = d_tx; a.var = d_variance; a.rx = d_rx; a.n_sym = n_sym; a.seed = seed; a.first_symbol = first_symbol;
    a.variance = variance; // (not read when the array is given)
    hipError_t e = nrldpc::launch_awgn(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "AWGN kernel launch");
    return NRLDPC_OK;
}

} // extern "C"
namespace nrldpc { // nrldpc_channel.hip (declared here, not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id)
hipError_t launch_payload_bits(uint64_t seed, uint64_t first_block, int32_t n_tb, int32_t A, uint8_t* out, hipStream_t stream);
}
extern "C" {

int nrldpc_payload_bits_dev(uint64_t seed, uint64_t first_block, int32_t n_tb, int32_t A, uint8_t* d_a, void* stream) {
    if (n_tb < 0 || A < 1) return fail(NRLDPC_ERR_ARG, "n_tb must be non-negative and A positive");
    if (n_tb == 0) return NRLDPC_OK;
    if (!d_a) return fail(NRLDPC_ERR_ARG, "null pointer");
    hipError_t e = nrldpc::launch_payload_bits(seed, first_block, n_tb, A, d_a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "payload kernel launch");
    return NRLDPC_OK;
}

int nrldpc_encode_dev(nrldpc_handle h, const uint8_t* d_info, int32_t batch, uint8_t* d_cw, void* stream) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    if (batch < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return NRLDPC_OK;
    if (!d_info || !d_cw) return fail(NRLDPC_ERR_ARG, "null info/cw pointer");
    DEVICE_SCOPE(h);
    return encode_launch(h, d_info, batch, d_cw, static_cast<hipStream_t>(stream));
}

int nrldpc_encode(nrldpc_handle h, const uint8_t* info, int32_t batch, uint8_t* cw) {
    if (!h) return fail(NRLDPC_ERR_ARG, "null handle");
    if (batch < 0) return fail(NRLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return NRLDPC_OK;
    if (!info || !cw) return fail(NRLDPC_ERR_ARG, "null info/cw pointer");
    DEVICE_SCOPE(h);
    const nrldpc::Schedule& s = h->sched;
    const size_t ncw = (size_t)s.g.ncols * s.Z, K = (size_t)s.g.kb * s.Z;
    HIP_TRY(h->s_bits.reserve((size_t)batch * K));
    HIP_TRY(h->s_hard.reserve((size_t)batch * ncw));
    HIP_TRY(hipMemcpyAsync(h->s_bits.p, info, (size_t)batch * K, hipMemcpyHostToDevice, nullptr));
    int rc = encode_launch(h, h->s_bits.p, batch, h->s_hard.p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(cw, h->s_hard.p, (size_t)batch * ncw, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NRLDPC_OK;
}

} // extern "C"

// ---- mixed transport-block batches (nrldpc_mix_*; kernels: nrldpc_mix.hip, tables and mapping: nrldpc_mix.h) -------------------------
static_assert(sizeof(nrldpc_mix_offsets) == 56, "nrldpc_mix_offsets: the size include/nrldpc.h states");
static_assert(nrldpc::MIX_FIELDS * sizeof(int64_t) == sizeof(nrldpc_mix_offsets), "one int64 per packed array, in the order of the MIX_* fields");

struct nrldpc_mix {
    int32_t n = 0, device_id = 0;
    std::vector<nrldpc_mix_offsets> off; // n + 1
    int64_t size_g = 0, size_harq = 0, size_cw = 0, size_c_hat = 0, size_cb = 0, size_b_hat = 0, size_tb = 0; // elements in use (sum over configurations)
    const int64_t* tb_offs = nullptr;    // device, [n]: off[i].tb (the d_new addressing of the HARQ rate recovery)
    char* blob = nullptr;                // every device table, one allocation, written once by nrldpc_mix_create
    nrldpc::MixRmLaunch rm{};
    nrldpc::MixCrcLaunch crc{};
    nrldpc::MixSkipLaunch skip{};        // nrldpc_mix_pending_dev / _gather_cw_dev / _scatter_hard_dev: the records; prefix, n_wg and esize per call
    const int32_t* skip_prefix[3] = {nullptr, nullptr, nullptr}; // device, [n + 1] each: the grids over f32 rows, f16 rows, hard-bit rows
    int32_t skip_wg[3] = {0, 0, 0};
};

namespace {

// everything the plan needs, on the host: offsets, records, tables.  No device call.
struct MixHost {
    std::vector<nrldpc_mix_offsets> off;
    std::vector<nrldpc::MixRmRec> rm;
    std::vector<nrldpc::MixCrcRec> crc;
    std::vector<int32_t> rm_prefix, tb_prefix, e_tab, off_tab;
    std::vector<nrldpc::MixSkipRec> skip;
    std::vector<int32_t> skip_prefix[3]; // f32 rows, f16 rows, hard-bit rows
    int64_t used[nrldpc::MIX_FIELDS] = {0, 0, 0, 0, 0, 0, 0};
    int32_t k_max = 0, c_max = 0;
};

int mix_fail_at(int rc, int i) {
    g_err += " (configuration " + std::to_string(i) + ")";
    return rc;
}

// the checks of the single-configuration calls on one block of a mix, with their texts: check_tb_params, fill_rm_blocks, the CRC stage's own
int mix_check_cfg(const nrldpc_tb_params* q, int32_t n_tb, int i, nrldpc::RmExArgs& blocks) {
    int rc = check_tb_params(q);
    if (rc) return mix_fail_at(rc, i);
    rc = fill_rm_blocks(q, 0, blocks); // (E_r and the offsets of the code blocks inside a row of g_tilde)
    if (rc) return mix_fail_at(rc, i);
    if ((q->tb_crc_len != 16 && q->tb_crc_len != 24) || (q->cb_crc_len != 0 && q->cb_crc_len != 24))
        return mix_fail_at(fail(NRLDPC_ERR_UNSUPPORTED, "CRC lengths must be 16/24 (TB) and 0/24 (CB)"), i);
    if (q->B != q->A + q->tb_crc_len || q->C * (q->K_prime - q->cb_crc_len) != q->B)
        return mix_fail_at(fail(NRLDPC_ERR_ARG, "B must equal A + L and C*(K' - L_cb)"), i);
    if (n_tb < 0) return mix_fail_at(fail(NRLDPC_ERR_ARG, "negative batch"), i);
    return NRLDPC_OK;
}

int mix_build(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, bool tables, MixHost& m) {
    if (n < 0) return fail(NRLDPC_ERR_ARG, "negative configuration count");
    if (n > 0 && (!p || !n_tb)) return fail(NRLDPC_ERR_ARG, "null array");
    m.off.assign((size_t)n + 1, nrldpc_mix_offsets{0, 0, 0, 0, 0, 0, 0});
    m.rm_prefix.assign((size_t)n + 1, 0);
    m.tb_prefix.assign((size_t)n + 1, 0);
    if (tables) { m.rm.resize(n); m.crc.resize(n); }
    int64_t wg = 0, tbs = 0;
    for (int i = 0; i < n; ++i) {
        const nrldpc_tb_params* q = p + i;
        nrldpc::RmExArgs blocks;
        const int rc = mix_check_cfg(q, n_tb[i], i, blocks);
        if (rc) return rc;
        const int32_t ncwz = 2 * q->Z + q->N;
        int64_t s[nrldpc::MIX_FIELDS];
        nrldpc::mix_sizes(n_tb[i], q->C, q->G, q->N_cb, ncwz, q->K, q->B, s);
        const int64_t* cur = &m.off[i].g;
        int64_t* next = &m.off[i + 1].g;
        for (int k = 0; k < nrldpc::MIX_FIELDS; ++k) { next[k] = nrldpc::mix_round_up(cur[k] + s[k]); m.used[k] += s[k]; }
        const int32_t per = nrldpc::mix_rm_wg_per_cb(ncwz);
        wg += (int64_t)n_tb[i] * q->C * per;
        tbs += n_tb[i];
        if (wg > INT32_MAX || tbs > INT32_MAX) return fail(NRLDPC_ERR_UNSUPPORTED, "the mix is too large for one launch");
        m.rm_prefix[i + 1] = (int32_t)wg;
        m.tb_prefix[i + 1] = (int32_t)tbs;
        if (!tables) continue;
        if (n_tb[i] > 0) { m.k_max = std::max(m.k_max, q->K); m.c_max = std::max(m.c_max, q->C); }
        nrldpc::MixRmRec& r = m.rm[i];
        memset(&r, 0, sizeof r);
        r.g_off = cur[nrldpc::MIX_G]; r.harq_off = cur[nrldpc::MIX_HARQ]; r.cw_off = cur[nrldpc::MIX_CW];
        r.n_tb = n_tb[i]; r.C = q->C; r.G = q->G; r.Z = q->Z; r.K = q->K; r.Kp = q->K_prime; r.N = q->N; r.N_cb = q->N_cb;
        r.k0 = q->k_0; r.Qm = q->Q_m;
        // the launch rule of the single-configuration calls without its environment knobs; the mix has no input-driven form
        // (asked without a buffer the rule answers general or plain gather) and takes `echo` in its place
        const nrldpc::RmRule rule = nrldpc::rm_launch_rule(nrldpc::RmGeom(q->Z, q->K, q->K_prime, q->N_cb, q->k_0), q->E_r, q->C, q->Q_m, q->N, false);
        r.form = rule.form;
        r.echo = rule.echo;
        r.e_base = (int32_t)m.e_tab.size();
        r.wg_per_cb = per;
        for (int b = 0; b < q->C; ++b) { m.e_tab.push_back(blocks.E[b]); m.off_tab.push_back(blocks.off[b]); }
        nrldpc::MixCrcRec& c = m.crc[i];
        memset(&c, 0, sizeof c);
        c.c_hat_off = cur[nrldpc::MIX_C_HAT]; c.b_hat_off = cur[nrldpc::MIX_B_HAT]; c.cb_off = cur[nrldpc::MIX_CB]; c.tb_off = cur[nrldpc::MIX_TB];
        c.C = q->C; c.K = q->K; c.Kp = q->K_prime; c.Lcb = q->cb_crc_len; c.A = q->A; c.B = q->B;
        const int pay = q->K_prime - q->cb_crc_len;
        make_crc_plan(&c.tb, crc_poly_for(q->tb_crc_len, false), q->tb_crc_len, pay, pay, pay);
        make_crc_plan(&c.cb, crc_poly_for(24, true), 24, q->K_prime, 0, 0);
    }
    if (tables) {
        // the pending / gather / scatter stages: a record per configuration and a grid per row type, sized for every row.  No grid exceeds
        // the rate-recovery grid checked above (8192 bytes of f32 are its 2048 positions; f16 and hard-bit rows are shorter).
        static_assert(nrldpc::MIX_SKIP_CHUNK == 4 * nrldpc::MIX_RM_WG, "the f32 gather grid is the rate-recovery grid");
        const int32_t esize[3] = {nrldpc::MIX_SKIP_ROW_F32, nrldpc::MIX_SKIP_ROW_F16, nrldpc::MIX_SKIP_ROW_HARD};
        m.skip.resize(n);
        for (int k = 0; k < 3; ++k) m.skip_prefix[k].assign((size_t)n + 1, 0);
        for (int i = 0; i < n; ++i) {
            nrldpc::MixSkipRec& s = m.skip[i];
            memset(&s, 0, sizeof s);
            s.cw_off = m.off[i].cw; s.c_hat_off = m.off[i].c_hat; s.cb_off = m.off[i].cb; s.tb_off = m.off[i].tb;
            s.n_cb = n_tb[i] * p[i].C; s.C = p[i].C; s.N_cw = 2 * p[i].Z + p[i].N; s.K = p[i].K;
            for (int k = 0; k < 3; ++k) {
                const int64_t wgs = m.skip_prefix[k][i] + (int64_t)s.n_cb * nrldpc::mix_skip_chunks(nrldpc::mix_skip_row_bytes(s, esize[k]));
                if (wgs > INT32_MAX) return fail(NRLDPC_ERR_UNSUPPORTED, "the mix is too large for one launch");
                m.skip_prefix[k][i + 1] = (int32_t)wgs;
            }
        }
    }
    return NRLDPC_OK;
}

} // namespace

extern "C" {

int nrldpc_mix_layout(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, nrldpc_mix_offsets* off) {
    NRLDPC_API_BEGIN
    if (n >= 0 && !off) return fail(NRLDPC_ERR_ARG, "null array");
    MixHost m;
    int rc = mix_build(n, p, n_tb, false, m);
    if (rc) return rc;
    memcpy(off, m.off.data(), m.off.size() * sizeof(nrldpc_mix_offsets));
    return NRLDPC_OK;
    NRLDPC_API_END
}

void nrldpc_mix_destroy(nrldpc_mix_handle m) {
    if (!m) return;
    if (m->blob) { DeviceScope scope(m->device_id); (void)hipFree(m->blob); }
    delete m;
}

int nrldpc_mix_create(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int32_t device_id, nrldpc_mix_handle* out) {
    NRLDPC_API_BEGIN
    if (!out) return fail(NRLDPC_ERR_ARG, "null out");
    *out = nullptr;
    MixHost mh;
    int rc = mix_build(n, p, n_tb, true, mh);
    if (rc) return rc;
    const bool empty = n == 0 || mh.tb_prefix[n] == 0; // an empty plan: no tables, no launches, no device call at all
    if (!empty) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
            return fail(NRLDPC_ERR_HIP, "no HIP device available (this library has no CPU path)");
        if (device_id < 0 || device_id >= ndev) return fail(NRLDPC_ERR_ARG, "device_id out of range");
    }
    nrldpc_mix* m = new (std::nothrow) nrldpc_mix();
    if (!m) return fail(NRLDPC_ERR_NOMEM, "host allocation failed");
    m->n = n; m->device_id = device_id; m->off = mh.off;
    m->size_g = mh.used[nrldpc::MIX_G]; m->size_harq = mh.used[nrldpc::MIX_HARQ]; m->size_cw = mh.used[nrldpc::MIX_CW];
    m->size_c_hat = mh.used[nrldpc::MIX_C_HAT]; m->size_cb = mh.used[nrldpc::MIX_CB]; m->size_b_hat = mh.used[nrldpc::MIX_B_HAT]; m->size_tb = mh.used[nrldpc::MIX_TB];
    m->rm.n = n; m->rm.n_wg = mh.rm_prefix[n];
    m->crc.n = n; m->crc.n_tb_total = mh.tb_prefix[n];
    m->crc.k_max = mh.k_max; m->crc.c_max = mh.c_max; m->crc.waves = mh.c_max < 4 ? (mh.c_max < 1 ? 1 : mh.c_max) : 4;
    if (empty) { *out = m; return NRLDPC_OK; }
    // one allocation, every table at a multiple of 16 bytes, uploaded synchronously and never written again
    auto pad16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_rm = 0, o_crc = o_rm + pad16(mh.rm.size() * sizeof(nrldpc::MixRmRec)), o_rp = o_crc + pad16(mh.crc.size() * sizeof(nrldpc::MixCrcRec)),
                 o_tp = o_rp + pad16(mh.rm_prefix.size() * 4), o_e = o_tp + pad16(mh.tb_prefix.size() * 4), o_o = o_e + pad16(mh.e_tab.size() * 4),
                 o_tbo = o_o + pad16(mh.off_tab.size() * 4), o_sk = o_tbo + pad16((size_t)n * 8), o_sp = o_sk + pad16(mh.skip.size() * sizeof(nrldpc::MixSkipRec)),
                 sp_len = pad16(((size_t)n + 1) * 4), total = o_sp + 3 * sp_len;
    std::vector<char> img(total, 0);
    memcpy(img.data() + o_rm, mh.rm.data(), mh.rm.size() * sizeof(nrldpc::MixRmRec));
    memcpy(img.data() + o_crc, mh.crc.data(), mh.crc.size() * sizeof(nrldpc::MixCrcRec));
    memcpy(img.data() + o_rp, mh.rm_prefix.data(), mh.rm_prefix.size() * 4);
    memcpy(img.data() + o_tp, mh.tb_prefix.data(), mh.tb_prefix.size() * 4);
    memcpy(img.data() + o_e, mh.e_tab.data(), mh.e_tab.size() * 4);
    memcpy(img.data() + o_o, mh.off_tab.data(), mh.off_tab.size() * 4);
    for (int i = 0; i < n; ++i) memcpy(img.data() + o_tbo + (size_t)i * 8, &mh.off[i].tb, 8);
    memcpy(img.data() + o_sk, mh.skip.data(), mh.skip.size() * sizeof(nrldpc::MixSkipRec));
    for (int k = 0; k < 3; ++k) memcpy(img.data() + o_sp + k * sp_len, mh.skip_prefix[k].data(), mh.skip_prefix[k].size() * 4);
    DeviceScope scope(device_id);
    hipError_t e = scope.err;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->blob), total);
    if (e == hipSuccess) e = hipMemcpy(m->blob, img.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { nrldpc_mix_destroy(m); return hipfail(e, "mix plan tables"); }
    m->rm.recs = reinterpret_cast<const nrldpc::MixRmRec*>(m->blob + o_rm);
    m->crc.recs = reinterpret_cast<const nrldpc::MixCrcRec*>(m->blob + o_crc);
    m->rm.prefix = reinterpret_cast<const int32_t*>(m->blob + o_rp);
    m->crc.prefix = reinterpret_cast<const int32_t*>(m->blob + o_tp);
    m->rm.e_tab = reinterpret_cast<const int32_t*>(m->blob + o_e);
    m->rm.off_tab = reinterpret_cast<const int32_t*>(m->blob + o_o);
    m->tb_offs = reinterpret_cast<const int64_t*>(m->blob + o_tbo);
    m->skip.recs = reinterpret_cast<const nrldpc::MixSkipRec*>(m->blob + o_sk);
    m->skip.n = n;
    for (int k = 0; k < 3; ++k) {
        m->skip_prefix[k] = reinterpret_cast<const int32_t*>(m->blob + o_sp + k * sp_len);
        m->skip_wg[k] = mh.skip_prefix[k][n];
    }
    *out = m;
    return NRLDPC_OK;
    NRLDPC_API_END
}

int nrldpc_mix_rate_recover_dev(nrldpc_mix_handle m, const void* d_g_tilde, int32_t in_dtype, void* d_harq, int32_t harq_dtype,
                                void* d_cw_llr, int32_t out_dtype, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    auto known = [](int32_t d) { return d == NRLDPC_LLR_F32 || d == NRLDPC_LLR_F16; };
    if (!known(in_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "in_dtype must be f32 or f16");
    if (d_harq && !known(harq_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "harq_dtype must be f32 or f16");
    if (!known(out_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "out_dtype must be f32 or f16");
    if ((m->size_cw > 0 && !d_cw_llr) || (m->size_g > 0 && !d_g_tilde)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->rm.n_wg == 0) return NRLDPC_OK;
    nrldpc::MixRmLaunch a = m->rm; // (a copy: calls in flight on several streams share the plan, never a launch block)
    a.g = d_g_tilde; a.harq = d_harq; a.out = d_cw_llr;
    a.in_f16 = in_dtype == NRLDPC_LLR_F16; a.harq_f16 = d_harq && harq_dtype == NRLDPC_LLR_F16; a.out_f16 = out_dtype == NRLDPC_LLR_F16;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_rate_recover(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix rate-recovery kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_crc_check_dev(nrldpc_mix_handle m, const uint8_t* d_c_hat, uint8_t* d_b_hat, int32_t* d_ok, int32_t* d_cb_pass, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if ((m->size_c_hat > 0 && !d_c_hat) || (m->size_b_hat > 0 && !d_b_hat) || (m->size_tb > 0 && !d_ok)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->crc.n_tb_total == 0) return NRLDPC_OK;
    nrldpc::MixCrcLaunch a = m->crc;
    a.c_hat = d_c_hat; a.b_hat = d_b_hat; a.ok = d_ok; a.cb_pass = d_cb_pass;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_crc_check(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix CRC kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_rate_recover_harq_dev(nrldpc_mix_handle m, const void* d_g_tilde, int32_t in_dtype, void* d_harq, int32_t harq_dtype,
                                     void* d_cw_llr, int32_t out_dtype, const uint8_t* d_new, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    auto known = [](int32_t d) { return d == NRLDPC_LLR_F32 || d == NRLDPC_LLR_F16; };
    if (!known(in_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "in_dtype must be f32 or f16");
    if (!known(harq_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "harq_dtype must be f32 or f16");
    if (!known(out_dtype)) return fail(NRLDPC_ERR_UNSUPPORTED, "out_dtype must be f32 or f16");
    if ((m->size_cw > 0 && !d_cw_llr) || (m->size_g > 0 && !d_g_tilde) || (m->size_harq > 0 && !d_harq)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->rm.n_wg == 0) return NRLDPC_OK;
    nrldpc::MixRmHarqLaunch a;
    a.b = m->rm;
    a.b.g = d_g_tilde; a.b.harq = d_harq; a.b.out = d_cw_llr;
    a.b.in_f16 = in_dtype == NRLDPC_LLR_F16; a.b.harq_f16 = harq_dtype == NRLDPC_LLR_F16; a.b.out_f16 = out_dtype == NRLDPC_LLR_F16;
    a.tb_offs = m->tb_offs; a.is_new = d_new;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    // no flags: every transport block continues -- that IS nrldpc_mix_rate_recover_dev, and its kernel is launched
    hipError_t e = d_new ? nrldpc::launch_mix_rate_recover_harq(a, static_cast<hipStream_t>(stream))
                         : nrldpc::launch_mix_rate_recover(a.b, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix rate-recovery kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_crc_check_harq_dev(nrldpc_mix_handle m, const uint8_t* d_c_hat, uint8_t* d_b_hat, int32_t* d_ok, int32_t* d_cb_pass,
                                  const uint8_t* d_cbgti, const uint8_t* d_new, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if ((m->size_c_hat > 0 && !d_c_hat) || (m->size_b_hat > 0 && !d_b_hat) || (m->size_tb > 0 && !d_ok)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->size_cb > 0 && !d_cb_pass) return fail(NRLDPC_ERR_ARG, "the sticky code-block flags (d_cb_pass) are required");
    if (m->crc.n_tb_total == 0) return NRLDPC_OK;
    nrldpc::MixCrcHarqLaunch a;
    a.b = m->crc;
    a.b.c_hat = d_c_hat; a.b.b_hat = d_b_hat; a.b.ok = d_ok; a.b.cb_pass = d_cb_pass;
    a.cbgti = d_cbgti; a.is_new = d_new;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_crc_check_harq(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix CRC kernel launch");
    return NRLDPC_OK;
}

// ---- HARQ steps that decode only the pending code blocks (kernels: nrldpc_mix_skip.hip; the rule and the mapping: nrldpc_mix_skip.h) ----
int nrldpc_mix_pending_dev(nrldpc_mix_handle m, int32_t rule, const int32_t* d_cb_pass, const int32_t* d_ok, const uint8_t* d_cbgti,
                           const uint8_t* d_new, int32_t* d_index, int32_t* d_count, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (rule != NRLDPC_MIX_SKIP_UNSCHEDULED && rule != NRLDPC_MIX_SKIP_SETTLED)
        return fail(NRLDPC_ERR_UNSUPPORTED, "rule must be NRLDPC_MIX_SKIP_UNSCHEDULED or NRLDPC_MIX_SKIP_SETTLED");
    if (m->size_cb == 0) return NRLDPC_OK; // the empty plan: no tables, no launch
    if (!d_index || !d_count) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (rule == NRLDPC_MIX_SKIP_SETTLED && (!d_cb_pass || !d_ok)) return fail(NRLDPC_ERR_ARG, "the settled rule needs d_cb_pass and d_ok");
    nrldpc::MixSkipState s;
    s.cb_pass = d_cb_pass; s.ok = d_ok; s.cbgti = d_cbgti; s.is_new = d_new;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_skip_pending(m->skip, rule, s, d_index, d_count, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix pending kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_gather_cw_dev(nrldpc_mix_handle m, const void* d_cw_llr, int32_t dtype, const int32_t* d_index, const int32_t* d_count,
                             void* d_cw_dense, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (dtype != NRLDPC_LLR_F32 && dtype != NRLDPC_LLR_F16) return fail(NRLDPC_ERR_UNSUPPORTED, "dtype must be f32 or f16");
    if (m->size_cb == 0) return NRLDPC_OK;
    if (!d_cw_llr || !d_index || !d_count || !d_cw_dense) return fail(NRLDPC_ERR_ARG, "null pointer");
    const int k = dtype == NRLDPC_LLR_F32 ? 0 : 1;
    nrldpc::MixSkipLaunch a = m->skip; // (a copy: calls in flight on several streams share the plan, never a launch block)
    a.prefix = m->skip_prefix[k]; a.n_wg = m->skip_wg[k]; a.esize = k == 0 ? nrldpc::MIX_SKIP_ROW_F32 : nrldpc::MIX_SKIP_ROW_F16;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_skip_gather(a, d_cw_llr, d_index, d_count, d_cw_dense, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix gather kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_scatter_hard_dev(nrldpc_mix_handle m, const uint8_t* d_c_hat_dense, const int32_t* d_iters_dense, const int32_t* d_index,
                                const int32_t* d_count, uint8_t* d_c_hat, int32_t* d_iters, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (m->size_cb == 0) return NRLDPC_OK;
    if (!d_c_hat_dense || !d_index || !d_count || !d_c_hat) return fail(NRLDPC_ERR_ARG, "null pointer");
    nrldpc::MixSkipLaunch a = m->skip;
    a.prefix = m->skip_prefix[2]; a.n_wg = m->skip_wg[2]; a.esize = nrldpc::MIX_SKIP_ROW_HARD;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_skip_scatter(a, d_c_hat_dense, d_iters_dense, d_index, d_count, d_c_hat, d_iters, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix scatter kernel launch");
    return NRLDPC_OK;
}

} // extern "C"

// ---- mixed transport-block batches, transmit side (nrldpc_mix_tx_*; kernels: nrldpc_mix_tx.hip, tables and mapping: nrldpc_mix_tx.h) ----
// A type of its own: the receive plan nrldpc_mix, its blob and its records are untouched.
struct nrldpc_mix_tx {
    int32_t n = 0, device_id = 0;
    std::vector<nrldpc_mix_offsets> off; // n + 1: the receive layout's (c = c_hat, codeword bytes = cw, rate-matched bits = g)
    std::vector<int64_t> a_off;          // n + 1: the payload array
    std::vector<int32_t> bg, Z, n_cw;    // per configuration: what its encoder handle must be, and its codewords n_tb * C
    int64_t size_a = 0, size_c = 0, size_cw = 0, size_g = 0; // elements in use (sum over configurations)
    char* blob = nullptr;                // every device table, one allocation, written once by nrldpc_mix_tx_create
    nrldpc::MixTxCrcLaunch crc{};
    nrldpc::MixTxRmLaunch rm{};
    nrldpc::MixTxEncLaunch enc{};        // nrldpc_mix_tx_encode_all_dev
    nrldpc::MixMcPayLaunch pay{};        // nrldpc_mix_tx_payload_dev
    nrldpc::MixMcOutLaunch outc{};       // nrldpc_mix_tx_outcome_dev (its transport-block prefix is the attach stage's)
};

namespace {

struct MixTxHost {
    std::vector<nrldpc_mix_offsets> off;
    std::vector<int64_t> a_off;
    std::vector<nrldpc::MixTxRmRec> rm;
    std::vector<nrldpc::MixTxCrcRec> crc;
    std::vector<int32_t> rm_prefix, tb_prefix, e_tab, off_tab;
    int64_t used_a = 0, used_c = 0, used_cw = 0, used_g = 0;
    int32_t k_max = 0, c_max = 0;
    // the one-launch encoder: records, workgroup prefix, the base-graph tables of every distinct (BG, Z_c), the launch's LDS size
    std::vector<nrldpc::MixTxEncRec> enc;
    std::vector<int32_t> enc_prefix, enc_first; // enc_first: the first configuration of each distinct (BG, Z_c)
    std::vector<uint8_t> enc_tab;
    int64_t enc_lds = 0;
    // the Monte-Carlo stages (nrldpc_mix_mc.h): records and the payload grid's workgroup prefix
    std::vector<nrldpc::MixMcRec> mc;
    std::vector<int32_t> pay_prefix;
};

// the encoder record of one non-empty configuration: sizes, waves per codeword, and -- once per distinct (BG, Z_c) -- the solve order
// and the tables EncArgs points to (row_ptr, col, shift reduced mod Z) appended to m.enc_tab
int mix_tx_enc_fill(int32_t bg, int32_t Z, int32_t i, MixTxHost& m) {
    nrldpc::MixTxEncRec& en = m.enc[i];
    nrldpc::BaseGraph g;
    const int ils = nrldpc::set_index(Z);
    if (!nrldpc::base_graph(bg, &g) || ils < 0) return fail(NRLDPC_ERR_UNSUPPORTED, "invalid BG / lifting size");
    en.Z = Z; en.kb = g.kb; en.nrows = g.nrows; en.ncols = g.ncols; en.nnz = g.nnz;
    en.nwc = nrldpc::mix_tx_enc_nwc(bg, Z);
    const int64_t lds = nrldpc::mix_tx_enc_lds_bytes(nrldpc::mix_tx_enc_layout(Z, g.kb, g.nrows, g.nnz), en.nwc);
    if (lds > 64 * 1024) return fail(NRLDPC_ERR_UNSUPPORTED, "the encoder's LDS does not fit a workgroup");
    m.enc_lds = std::max(m.enc_lds, lds);
    for (int32_t k : m.enc_first) {
        const nrldpc::MixTxEncRec& f = m.enc[k];
        if (f.kb == en.kb && f.Z == Z) { // the same (BG, Z_c): one table, one solve order
            en.row_ptr_off = f.row_ptr_off; en.shift_off = f.shift_off; en.col_off = f.col_off; en.ord = f.ord;
            return NRLDPC_OK;
        }
    }
    std::vector<int32_t> shift((size_t)g.nnz);
    for (int e = 0; e < g.nnz; ++e) shift[(size_t)e] = g.raw_shift(ils, e) % Z;
    if (!derive_encoder_order(g, shift.data(), &en.ord)) return fail(NRLDPC_ERR_UNSUPPORTED, "base graph core is not dual-diagonal");
    const size_t base = m.enc_tab.size();
    if (base + (size_t)nrldpc::mix_tx_enc_tab_bytes(g.nrows, g.nnz) > (size_t)INT32_MAX) return fail(NRLDPC_ERR_UNSUPPORTED, "the mix is too large for one launch");
    nrldpc::mix_tx_enc_tab_place((int32_t)base, en);
    m.enc_tab.resize(base + (size_t)nrldpc::mix_tx_enc_tab_bytes(g.nrows, g.nnz), 0);
    memcpy(m.enc_tab.data() + en.row_ptr_off, g.row_ptr, (size_t)(g.nrows + 1) * 2);
    std::vector<uint16_t> sh16(shift.begin(), shift.end());
    memcpy(m.enc_tab.data() + en.shift_off, sh16.data(), (size_t)g.nnz * 2);
    memcpy(m.enc_tab.data() + en.col_off, g.col, (size_t)g.nnz);
    m.enc_first.push_back(i);
    return NRLDPC_OK;
}

// everything the transmit plan needs, on the host.  No device call.  The refusals of mix_build, then the transmit stages' own.
int mix_tx_build(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, bool tables, MixTxHost& m) {
    if (n < 0) return fail(NRLDPC_ERR_ARG, "negative configuration count");
    if (n > 0 && (!p || !n_tb)) return fail(NRLDPC_ERR_ARG, "null array");
    m.off.assign((size_t)n + 1, nrldpc_mix_offsets{0, 0, 0, 0, 0, 0, 0});
    m.a_off.assign((size_t)n + 1, 0);
    m.rm_prefix.assign((size_t)n + 1, 0);
    m.tb_prefix.assign((size_t)n + 1, 0);
    m.enc_prefix.assign((size_t)n + 1, 0);
    m.pay_prefix.assign((size_t)n + 1, 0);
    if (tables) { m.rm.resize(n); m.crc.resize(n); m.enc.resize(n); m.mc.resize(n); }
    int64_t wg = 0, wg_rx = 0, tbs = 0, wg_enc = 0, wg_pay = 0;
    for (int i = 0; i < n; ++i) {
        const nrldpc_tb_params* q = p + i;
        nrldpc::RmExArgs blocks;
        const int rc = mix_check_cfg(q, n_tb[i], i, blocks);
        if (rc) return rc;
        const int pay = q->K_prime - q->cb_crc_len;
        if (pay < q->tb_crc_len) return mix_fail_at(fail(NRLDPC_ERR_UNSUPPORTED, "code block shorter than the transport-block CRC"), i);
        if (q->Q_m != 1 && q->Q_m != 2 && q->Q_m != 4 && q->Q_m != 6 && q->Q_m != 8) return mix_fail_at(fail(NRLDPC_ERR_UNSUPPORTED, "Unsupported modulation"), i);
        const int32_t ncwz = 2 * q->Z + q->N;
        int64_t s[nrldpc::MIX_FIELDS];
        nrldpc::mix_sizes(n_tb[i], q->C, q->G, q->N_cb, ncwz, q->K, q->B, s);
        const int64_t* cur = &m.off[i].g;
        int64_t* next = &m.off[i + 1].g;
        for (int k = 0; k < nrldpc::MIX_FIELDS; ++k) next[k] = nrldpc::mix_round_up(cur[k] + s[k]);
        m.a_off[i + 1] = nrldpc::mix_tx_a_next(m.a_off[i], n_tb[i], q->A);
        m.used_a += (int64_t)n_tb[i] * q->A; m.used_c += s[nrldpc::MIX_C_HAT]; m.used_cw += s[nrldpc::MIX_CW]; m.used_g += s[nrldpc::MIX_G];
        int32_t e_max = 0;
        for (int b = 0; b < q->C; ++b) e_max = std::max(e_max, blocks.E[b]);
        const int32_t per = nrldpc::mix_tx_rm_wg_per_cb(e_max, q->Q_m);
        wg += (int64_t)n_tb[i] * q->C * per;
        wg_rx += (int64_t)n_tb[i] * q->C * nrldpc::mix_rm_wg_per_cb(ncwz); // (a plan nrldpc_mix_create refuses is refused here too)
        tbs += n_tb[i];
        const int64_t n_cw = (int64_t)n_tb[i] * q->C; // (below 2^31 once wg_rx is: a code block takes a receive workgroup at least)
        const int32_t nwc = nrldpc::mix_tx_enc_nwc(q->bg, q->Z), per_enc = nrldpc::mix_tx_enc_per_wg(nwc);
        wg_enc += (n_cw + per_enc - 1) / per_enc;
        wg_pay += nrldpc::mix_mc_pay_wgs(n_tb[i], q->A); // (A/1024 workgroups a block: fewer than wg_rx, so no plan is refused that was not)
        if (wg > INT32_MAX || wg_rx > INT32_MAX || tbs > INT32_MAX || wg_enc > INT32_MAX || wg_pay > INT32_MAX) return fail(NRLDPC_ERR_UNSUPPORTED, "the mix is too large for one launch");
        m.pay_prefix[i + 1] = (int32_t)wg_pay;
        m.rm_prefix[i + 1] = (int32_t)wg;
        m.tb_prefix[i + 1] = (int32_t)tbs;
        m.enc_prefix[i + 1] = (int32_t)wg_enc;
        if (!tables) continue;
        if (n_tb[i] > 0) { m.k_max = std::max(m.k_max, q->K); m.c_max = std::max(m.c_max, q->C); }
        nrldpc::MixTxRmRec& r = m.rm[i];
        memset(&r, 0, sizeof r);
        r.cw_off = cur[nrldpc::MIX_CW]; r.g_off = cur[nrldpc::MIX_G];
        r.n_tb = n_tb[i]; r.C = q->C; r.G = q->G; r.Z = q->Z; r.K = q->K; r.Kp = q->K_prime; r.N = q->N; r.N_cb = q->N_cb;
        r.k0 = q->k_0; r.Qm = q->Q_m;
        r.e_base = (int32_t)m.e_tab.size();
        r.wg_per_cb = per;
        for (int b = 0; b < q->C; ++b) { m.e_tab.push_back(blocks.E[b]); m.off_tab.push_back(blocks.off[b]); }
        nrldpc::MixTxCrcRec& c = m.crc[i];
        memset(&c, 0, sizeof c);
        c.g.a_off = m.a_off[i]; c.g.c_off = cur[nrldpc::MIX_C_HAT];
        c.g.C = q->C; c.g.K = q->K; c.g.Kp = q->K_prime; c.g.Lcb = q->cb_crc_len; c.g.A = q->A; c.g.B = q->B;
        // the plans of nrldpc_crc_attach_dev, not of the receive side: horner_tail for the shorter last segment, the code-block plan
        // over the payload K' - L_cb
        make_crc_plan(&c.tb, crc_poly_for(q->tb_crc_len, false), q->tb_crc_len, pay, pay, pay - q->tb_crc_len);
        make_crc_plan(&c.cb, crc_poly_for(24, true), 24, pay, 0, 0);
        nrldpc::MixTxEncRec& en = m.enc[i];
        memset(&en, 0, sizeof en);
        en.c_off = cur[nrldpc::MIX_C_HAT]; en.cw_off = cur[nrldpc::MIX_CW];
        en.n_cw = (int32_t)n_cw;
        nrldpc::MixMcRec& mc = m.mc[i];
        memset(&mc, 0, sizeof mc);
        mc.a_off = m.a_off[i]; mc.b_hat_off = cur[nrldpc::MIX_B_HAT]; mc.tb_off = cur[nrldpc::MIX_TB];
        mc.n_tb = n_tb[i]; mc.A = q->A; mc.B = q->B;
        if (n_cw > 0) { // (an empty configuration has no workgroup: its record is never read)
            const int rce = mix_tx_enc_fill(q->bg, q->Z, i, m);
            if (rce) return mix_fail_at(rce, i);
        }
    }
    return NRLDPC_OK;
}

} // namespace

extern "C" {

int nrldpc_mix_tx_layout(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int64_t* a_off) {
    NRLDPC_API_BEGIN
    if (n >= 0 && !a_off) return fail(NRLDPC_ERR_ARG, "null array");
    MixTxHost m;
    int rc = mix_tx_build(n, p, n_tb, false, m);
    if (rc) return rc;
    memcpy(a_off, m.a_off.data(), m.a_off.size() * sizeof(int64_t));
    return NRLDPC_OK;
    NRLDPC_API_END
}

void nrldpc_mix_tx_destroy(nrldpc_mix_tx_handle m) {
    if (!m) return;
    if (m->blob) { DeviceScope scope(m->device_id); (void)hipFree(m->blob); }
    delete m;
}

int nrldpc_mix_tx_create(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int32_t device_id, nrldpc_mix_tx_handle* out) {
    NRLDPC_API_BEGIN
    if (!out) return fail(NRLDPC_ERR_ARG, "null out");
    *out = nullptr;
    MixTxHost mh;
    int rc = mix_tx_build(n, p, n_tb, true, mh);
    if (rc) return rc;
    const bool empty = n == 0 || mh.tb_prefix[n] == 0; // an empty plan: no tables, no launches, no device call at all
    if (!empty) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
            return fail(NRLDPC_ERR_HIP, "no HIP device available (this library has no CPU path)");
        if (device_id < 0 || device_id >= ndev) return fail(NRLDPC_ERR_ARG, "device_id out of range");
    }
    nrldpc_mix_tx* m = new (std::nothrow) nrldpc_mix_tx();
    if (!m) return fail(NRLDPC_ERR_NOMEM, "host allocation failed");
    m->n = n; m->device_id = device_id; m->off = mh.off; m->a_off = mh.a_off;
    for (int i = 0; i < n; ++i) { m->bg.push_back(p[i].bg); m->Z.push_back(p[i].Z); m->n_cw.push_back(n_tb[i] * p[i].C); }
    m->size_a = mh.used_a; m->size_c = mh.used_c; m->size_cw = mh.used_cw; m->size_g = mh.used_g;
    m->rm.n = n; m->rm.n_wg = mh.rm_prefix[n];
    m->crc.n = n; m->crc.n_tb_total = mh.tb_prefix[n];
    m->crc.k_max = mh.k_max; m->crc.c_max = mh.c_max; m->crc.waves = nrldpc::mix_tx_waves(mh.c_max);
    m->enc.n = n; m->enc.n_wg = mh.enc_prefix[n]; m->enc.lds_bytes = (int32_t)mh.enc_lds;
    m->pay.n = n; m->pay.n_wg = mh.pay_prefix[n];
    m->outc.n = n; m->outc.n_tb_total = mh.tb_prefix[n];
    if (empty) { *out = m; return NRLDPC_OK; }
    // one allocation, every table at a multiple of 16 bytes, uploaded synchronously and never written again
    auto pad16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_rm = 0, o_crc = o_rm + pad16(mh.rm.size() * sizeof(nrldpc::MixTxRmRec)), o_rp = o_crc + pad16(mh.crc.size() * sizeof(nrldpc::MixTxCrcRec)),
                 o_tp = o_rp + pad16(mh.rm_prefix.size() * 4), o_e = o_tp + pad16(mh.tb_prefix.size() * 4), o_o = o_e + pad16(mh.e_tab.size() * 4),
                 o_er = o_o + pad16(mh.off_tab.size() * 4), o_ep = o_er + pad16(mh.enc.size() * sizeof(nrldpc::MixTxEncRec)),
                 o_et = o_ep + pad16(mh.enc_prefix.size() * 4), o_mc = o_et + pad16(mh.enc_tab.size()),
                 o_pp = o_mc + pad16(mh.mc.size() * sizeof(nrldpc::MixMcRec)), total = o_pp + pad16(mh.pay_prefix.size() * 4);
    std::vector<char> img(total, 0);
    memcpy(img.data() + o_rm, mh.rm.data(), mh.rm.size() * sizeof(nrldpc::MixTxRmRec));
    memcpy(img.data() + o_crc, mh.crc.data(), mh.crc.size() * sizeof(nrldpc::MixTxCrcRec));
    memcpy(img.data() + o_rp, mh.rm_prefix.data(), mh.rm_prefix.size() * 4);
    memcpy(img.data() + o_tp, mh.tb_prefix.data(), mh.tb_prefix.size() * 4);
    memcpy(img.data() + o_e, mh.e_tab.data(), mh.e_tab.size() * 4);
    memcpy(img.data() + o_o, mh.off_tab.data(), mh.off_tab.size() * 4);
    memcpy(img.data() + o_er, mh.enc.data(), mh.enc.size() * sizeof(nrldpc::MixTxEncRec));
    memcpy(img.data() + o_ep, mh.enc_prefix.data(), mh.enc_prefix.size() * 4);
    memcpy(img.data() + o_et, mh.enc_tab.data(), mh.enc_tab.size());
    memcpy(img.data() + o_mc, mh.mc.data(), mh.mc.size() * sizeof(nrldpc::MixMcRec));
    memcpy(img.data() + o_pp, mh.pay_prefix.data(), mh.pay_prefix.size() * 4);
    DeviceScope scope(device_id);
    hipError_t e = scope.err;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->blob), total);
    if (e == hipSuccess) e = hipMemcpy(m->blob, img.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { nrldpc_mix_tx_destroy(m); return hipfail(e, "mix transmit plan tables"); }
    m->rm.recs = reinterpret_cast<const nrldpc::MixTxRmRec*>(m->blob + o_rm);
    m->crc.recs = reinterpret_cast<const nrldpc::MixTxCrcRec*>(m->blob + o_crc);
    m->rm.prefix = reinterpret_cast<const int32_t*>(m->blob + o_rp);
    m->crc.prefix = reinterpret_cast<const int32_t*>(m->blob + o_tp);
    m->rm.e_tab = reinterpret_cast<const int32_t*>(m->blob + o_e);
    m->rm.off_tab = reinterpret_cast<const int32_t*>(m->blob + o_o);
    m->enc.recs = reinterpret_cast<const nrldpc::MixTxEncRec*>(m->blob + o_er);
    m->enc.prefix = reinterpret_cast<const int32_t*>(m->blob + o_ep);
    m->enc.tab = reinterpret_cast<const uint8_t*>(m->blob + o_et);
    m->pay.recs = m->outc.recs = reinterpret_cast<const nrldpc::MixMcRec*>(m->blob + o_mc);
    m->pay.prefix = reinterpret_cast<const int32_t*>(m->blob + o_pp);
    m->outc.tb_prefix = m->crc.prefix;
    *out = m;
    return NRLDPC_OK;
    NRLDPC_API_END
}

int nrldpc_mix_tx_crc_attach_dev(nrldpc_mix_tx_handle m, const uint8_t* d_a, uint8_t* d_c, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if ((m->size_a > 0 && !d_a) || (m->size_c > 0 && !d_c)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->crc.n_tb_total == 0) return NRLDPC_OK;
    nrldpc::MixTxCrcLaunch a = m->crc; // (a copy: calls in flight on several streams share the plan, never a launch block)
    a.a = d_a; a.c = d_c;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_tx_crc_attach(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix CRC attach kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_tx_encode_dev(nrldpc_mix_tx_handle m, const nrldpc_handle* h, const uint8_t* d_c, uint8_t* d_cw, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if ((m->size_c > 0 && !d_c) || (m->size_cw > 0 && !d_cw)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->crc.n_tb_total == 0) return NRLDPC_OK;
    if (!h) return fail(NRLDPC_ERR_ARG, "null array");
    for (int i = 0; i < m->n; ++i) { // every handle checked before the first launch
        if (m->n_cw[i] == 0) continue;
        if (!h[i]) return mix_fail_at(fail(NRLDPC_ERR_ARG, "null handle"), i);
        if (h[i]->cfg.bg != m->bg[i] || h[i]->cfg.Z != m->Z[i]) return mix_fail_at(fail(NRLDPC_ERR_ARG, "the handle's (BG, Z) is not the configuration's"), i);
        if (h[i]->cfg.device_id != m->device_id) return mix_fail_at(fail(NRLDPC_ERR_ARG, "the handle lives on another device than the plan"), i);
    }
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    for (int i = 0; i < m->n; ++i) {
        if (m->n_cw[i] == 0) continue;
        const int rc = encode_launch(h[i], d_c + m->off[i].c_hat, m->n_cw[i], d_cw + m->off[i].cw, static_cast<hipStream_t>(stream));
        if (rc) return mix_fail_at(rc, i);
    }
    return NRLDPC_OK;
}

// the encode stage in one launch (nrldpc_mix_tx_enc.hip): no handles, the plan's own tables
int nrldpc_mix_tx_encode_all_dev(nrldpc_mix_tx_handle m, const uint8_t* d_c, uint8_t* d_cw, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if ((m->size_c > 0 && !d_c) || (m->size_cw > 0 && !d_cw)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->enc.n_wg == 0) return NRLDPC_OK;
    nrldpc::MixTxEncLaunch a = m->enc; // (a copy: calls in flight on several streams share the plan, never a launch block)
    a.c = d_c; a.cw = d_cw;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_tx_encode(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix encode kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_tx_rate_match_dev(nrldpc_mix_tx_handle m, const uint8_t* d_cw, uint8_t* d_g, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if ((m->size_cw > 0 && !d_cw) || (m->size_g > 0 && !d_g)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->rm.n_wg == 0) return NRLDPC_OK;
    nrldpc::MixTxRmLaunch a = m->rm;
    a.cw = d_cw; a.g = d_g;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_tx_rate_match(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix rate-matching kernel launch");
    return NRLDPC_OK;
}

// ---- the Monte-Carlo loop's own two stages on the transmit plan (kernels: nrldpc_mix_mc.hip, records and mapping: nrldpc_mix_mc.h) ----
static_assert(sizeof(nrldpc_mix_draw) == 16, "nrldpc_mix_draw: the size include/nrldpc.h states");

int nrldpc_mix_tx_payload_dev(nrldpc_mix_tx_handle m, const nrldpc_mix_draw* d_draw, uint8_t* d_a, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (m->size_a > 0 && !d_a) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->pay.n_wg == 0) return NRLDPC_OK;
    if (!d_draw) return fail(NRLDPC_ERR_ARG, "null draw records");
    nrldpc::MixMcPayLaunch a = m->pay; // (a copy: calls in flight on several streams share the plan, never a launch block)
    a.draw = d_draw; a.a = d_a;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_mc_payload(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix payload kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_tx_outcome_dev(nrldpc_mix_tx_handle m, const uint8_t* d_a, const uint8_t* d_b_hat, const int32_t* d_ok, int32_t first,
                              uint8_t* d_a_hat, uint8_t* d_done, uint8_t* d_good, int32_t* d_left, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    // (a transport block has A >= 1 payload bytes and B > A bytes of b_hat: every array is non-empty exactly when the payload array is)
    if (m->size_a > 0 && (!d_a || !d_b_hat || !d_ok || !d_a_hat || !d_done || !d_good)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->outc.n_tb_total == 0) return NRLDPC_OK;
    nrldpc::MixMcOutLaunch a = m->outc;
    a.first = first; a.a = d_a; a.b_hat = d_b_hat; a.ok = d_ok; a.a_hat = d_a_hat; a.done = d_done; a.good = d_good; a.left = d_left;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_mc_outcome(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix outcome kernel launch");
    return NRLDPC_OK;
}

} // extern "C"

// ---- mixed transport-block batches, the channel leg (nrldpc_mix_chan_*; kernels: nrldpc_mix_chan.hip and nrldpc_mix_modem.hip, tables and
// mapping: nrldpc_mix_chan.h) ----
// A third plan type: the receive plan nrldpc_mix and the transmit plan nrldpc_mix_tx, their blobs and their records are untouched.
static_assert(sizeof(nrldpc_mix_chan_point) == 32, "nrldpc_mix_chan_point: the size include/nrldpc.h states");

struct nrldpc_mix_chan {
    int32_t n = 0, device_id = 0;
    int64_t size_g = 0, size_sym = 0;    // elements in use (sum over configurations): bits / LLRs, symbols
    char* blob = nullptr;                // every device table, one allocation, written once by nrldpc_mix_chan_create
    nrldpc::MixChanTables modem{};       // mapper and demapper: a thread per S symbols
    nrldpc::MixChanTables pair{};        // fused stage and stand-alone noise: a thread per aligned pair of the global symbol count
};

namespace {

struct MixChanHost {
    std::vector<int64_t> sym_off;
    std::vector<nrldpc::MixChanRec> recs;
    std::vector<int32_t> modem_prefix, pair_prefix;
    int64_t used_g = 0, used_sym = 0;
};

// everything the channel plan needs, on the host.  No device call.  The refusals of mix_build, then the modulation order.
int mix_chan_build(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, MixChanHost& m) {
    if (n < 0) return fail(NRLDPC_ERR_ARG, "negative configuration count");
    if (n > 0 && (!p || !n_tb)) return fail(NRLDPC_ERR_ARG, "null array");
    m.sym_off.assign((size_t)n + 1, 0);
    m.modem_prefix.assign((size_t)n + 1, 0);
    m.pair_prefix.assign((size_t)n + 1, 0);
    m.recs.resize(n);
    int64_t g_off = 0, wg_rx = 0, tbs = 0, wg_modem = 0, wg_pair = 0;
    for (int i = 0; i < n; ++i) {
        const nrldpc_tb_params* q = p + i;
        nrldpc::RmExArgs blocks;
        const int rc = mix_check_cfg(q, n_tb[i], i, blocks);
        if (rc) return rc;
        if (q->Q_m != 1 && q->Q_m != 2 && q->Q_m != 4 && q->Q_m != 6 && q->Q_m != 8) return mix_fail_at(fail(NRLDPC_ERR_UNSUPPORTED, "Unsupported modulation"), i);
        const int64_t bits = (int64_t)n_tb[i] * q->G, n_sym = bits / q->Q_m; // (G is a multiple of Q_m: every E_r is)
        nrldpc::MixChanRec& r = m.recs[i];
        memset(&r, 0, sizeof r);
        r.g_off = g_off; r.sym_off = m.sym_off[i]; r.n_sym = n_sym; r.Qm = q->Q_m;
        r.inv_norm = (float)(1.0 / std::sqrt(2.0 * kRailMeanSq[q->Q_m / 2]));
        g_off = nrldpc::mix_round_up(g_off + bits); // field g of nrldpc_mix_layout
        m.sym_off[i + 1] = nrldpc::mix_chan_sym_next(m.sym_off[i], n_sym);
        m.used_g += bits; m.used_sym += n_sym;
        wg_rx += (int64_t)n_tb[i] * q->C * nrldpc::mix_rm_wg_per_cb(2 * q->Z + q->N); // (a plan nrldpc_mix_create refuses is refused here too)
        tbs += n_tb[i];
        wg_modem += nrldpc::mix_chan_modem_wgs(n_sym, q->Q_m);
        wg_pair += nrldpc::mix_chan_pair_wgs(n_sym);
        if (wg_rx > INT32_MAX || tbs > INT32_MAX || wg_modem > INT32_MAX || wg_pair > INT32_MAX) return fail(NRLDPC_ERR_UNSUPPORTED, "the mix is too large for one launch");
        m.modem_prefix[i + 1] = (int32_t)wg_modem;
        m.pair_prefix[i + 1] = (int32_t)wg_pair;
    }
    return NRLDPC_OK;
}

} // namespace

extern "C" {

int nrldpc_mix_chan_layout(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int64_t* sym_off) {
    NRLDPC_API_BEGIN
    if (n >= 0 && !sym_off) return fail(NRLDPC_ERR_ARG, "null array");
    MixChanHost m;
    int rc = mix_chan_build(n, p, n_tb, m);
    if (rc) return rc;
    memcpy(sym_off, m.sym_off.data(), m.sym_off.size() * sizeof(int64_t));
    return NRLDPC_OK;
    NRLDPC_API_END
}

int nrldpc_mix_chan_point_set(float EsN0_dB, uint64_t seed, uint64_t first_symbol, nrldpc_mix_chan_point* out) {
    if (!out) return fail(NRLDPC_ERR_ARG, "null out");
    if (!(EsN0_dB > -60.0f && EsN0_dB < 80.0f)) return fail(NRLDPC_ERR_ARG, "EsN0_dB out of range");
    const double n0 = std::pow(10.0, -(double)EsN0_dB / 10.0); // the arithmetic of nrldpc_awgn_llr_dev, each field narrowed once
    out->variance = (float)n0;
    out->sigma = (float)std::sqrt(n0 / 2.0); out->inv_n0 = (float)(1.0 / n0);
    out->reserved = 0;
    out->seed = seed; out->first_symbol = first_symbol;
    return NRLDPC_OK;
}

void nrldpc_mix_chan_destroy(nrldpc_mix_chan_handle m) {
    if (!m) return;
    if (m->blob) { DeviceScope scope(m->device_id); (void)hipFree(m->blob); }
    delete m;
}

int nrldpc_mix_chan_create(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int32_t device_id, nrldpc_mix_chan_handle* out) {
    NRLDPC_API_BEGIN
    if (!out) return fail(NRLDPC_ERR_ARG, "null out");
    *out = nullptr;
    MixChanHost mh;
    int rc = mix_chan_build(n, p, n_tb, mh);
    if (rc) return rc;
    bool empty = true; // an empty plan: no tables, no launches, no device call at all
    for (int i = 0; i < n; ++i) empty = empty && n_tb[i] == 0;
    if (!empty) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
            return fail(NRLDPC_ERR_HIP, "no HIP device available (this library has no CPU path)");
        if (device_id < 0 || device_id >= ndev) return fail(NRLDPC_ERR_ARG, "device_id out of range");
    }
    nrldpc_mix_chan* m = new (std::nothrow) nrldpc_mix_chan();
    if (!m) return fail(NRLDPC_ERR_NOMEM, "host allocation failed");
    m->n = n; m->device_id = device_id;
    m->size_g = mh.used_g; m->size_sym = mh.used_sym;
    m->modem.n = m->pair.n = n;
    m->modem.n_wg = mh.modem_prefix[n]; m->pair.n_wg = mh.pair_prefix[n];
    if (empty) { *out = m; return NRLDPC_OK; }
    // one allocation, every table at a multiple of 16 bytes, uploaded synchronously and never written again
    auto pad16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_rec = 0, o_mp = o_rec + pad16(mh.recs.size() * sizeof(nrldpc::MixChanRec)), o_pp = o_mp + pad16(mh.modem_prefix.size() * 4),
                 total = o_pp + pad16(mh.pair_prefix.size() * 4);
    std::vector<char> img(total, 0);
    memcpy(img.data() + o_rec, mh.recs.data(), mh.recs.size() * sizeof(nrldpc::MixChanRec));
    memcpy(img.data() + o_mp, mh.modem_prefix.data(), mh.modem_prefix.size() * 4);
    memcpy(img.data() + o_pp, mh.pair_prefix.data(), mh.pair_prefix.size() * 4);
    DeviceScope scope(device_id);
    hipError_t e = scope.err;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->blob), total);
    if (e == hipSuccess) e = hipMemcpy(m->blob, img.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { nrldpc_mix_chan_destroy(m); return hipfail(e, "mix channel plan tables"); }
    m->modem.recs = m->pair.recs = reinterpret_cast<const nrldpc::MixChanRec*>(m->blob + o_rec);
    m->modem.prefix = reinterpret_cast<const int32_t*>(m->blob + o_mp);
    m->pair.prefix = reinterpret_cast<const int32_t*>(m->blob + o_pp);
    *out = m;
    return NRLDPC_OK;
    NRLDPC_API_END
}

int nrldpc_mix_chan_awgn_llr_dev(nrldpc_mix_chan_handle m, const uint8_t* d_g, const nrldpc_mix_chan_point* d_pt, float* d_g_tilde, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (m->size_g > 0 && (!d_g || !d_g_tilde)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->pair.n_wg == 0) return NRLDPC_OK;
    if (!d_pt) return fail(NRLDPC_ERR_ARG, "null operating points");
    nrldpc::MixChanLlrLaunch a; // (a launch block of the call's own: calls in flight on several streams share the plan, never a launch block)
    a.t = m->pair; a.pt = d_pt; a.g = d_g; a.llr = d_g_tilde;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_chan_awgn_llr(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix channel kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_chan_modulate_dev(nrldpc_mix_chan_handle m, const uint8_t* d_g, float* d_tx, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (m->size_g > 0 && (!d_g || !d_tx)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->modem.n_wg == 0) return NRLDPC_OK;
    nrldpc::MixChanModLaunch a;
    a.t = m->modem; a.g = d_g; a.tx = d_tx;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_chan_modulate(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix mapper kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_chan_awgn_dev(nrldpc_mix_chan_handle m, const float* d_tx, const nrldpc_mix_chan_point* d_pt, const float* d_variance,
                             float* d_rx, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (m->size_sym > 0 && (!d_tx || !d_rx)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->pair.n_wg == 0) return NRLDPC_OK;
    if (!d_pt) return fail(NRLDPC_ERR_ARG, "null operating points"); // (seed and first_symbol are read with the array too)
    nrldpc::MixChanAwgnLaunch a;
    a.t = m->pair; a.pt = d_pt; a.tx = d_tx; a.var = d_variance; a.rx = d_rx;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_chan_awgn(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix AWGN kernel launch");
    return NRLDPC_OK;
}

int nrldpc_mix_chan_demodulate_dev(nrldpc_mix_chan_handle m, const float* d_rx, int32_t method, const nrldpc_mix_chan_point* d_pt,
                                   const float* d_variance, void* d_out, int32_t out_dtype, void* stream) {
    if (!m) return fail(NRLDPC_ERR_ARG, "null mix plan");
    if (method != NRLDPC_DEMOD_LLR && method != NRLDPC_DEMOD_APPROX_LLR && method != NRLDPC_DEMOD_HARD)
        return fail(NRLDPC_ERR_UNSUPPORTED, "unknown decision method");
    const bool hard = method == NRLDPC_DEMOD_HARD;
    if (!hard && out_dtype != NRLDPC_LLR_F32 && out_dtype != NRLDPC_LLR_F16) return fail(NRLDPC_ERR_UNSUPPORTED, "out_dtype must be f32 or f16");
    if (m->size_sym > 0 && (!d_rx || !d_out)) return fail(NRLDPC_ERR_ARG, "null pointer");
    if (m->modem.n_wg == 0) return NRLDPC_OK;
    if (!hard && !d_variance && !d_pt) return fail(NRLDPC_ERR_ARG, "null operating points");
    nrldpc::MixChanDemodLaunch a;
    a.t = m->modem; a.pt = d_pt; a.rx = d_rx; a.var = d_variance; a.out = d_out; a.method = method; a.out_dtype = out_dtype;
    DeviceScope scope(m->device_id);
    if (scope.err != hipSuccess) return hipfail(scope.err, "hipSetDevice");
    hipError_t e = nrldpc::launch_mix_chan_demodulate(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "mix demapper kernel launch");
    return NRLDPC_OK;
}

} // extern "C"
