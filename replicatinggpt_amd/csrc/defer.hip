// charpt deferred work (defer.h; include/charpt.h "Deferred work"): the per-(device, stream) queues of
// split-K reduces, AdamW updates and column-sum reduces, what a persistent GEMM launch takes from them
// and what cg_flush_deferred launches.  Host code only: the kernels are reduce.hip's and adamw.hip's.
#include <map>

#include "defer.h"

namespace cg {
int g_adam_per_launch = 0;   // cg_set_tuning("adam_per_launch"): AdamW jobs one launch's free blocks take (0 = MAX_ADAM)
int g_red_side = 1;       // cg_set_tuning("red_side"): a part-filling persistent launch takes a pending reduce on extra blocks
int g_adam_batch = 1;     // cg_set_tuning("adam_batch"), A/B build only: the side blocks' AdamW chunks in flight per thread
int g_skip_splitk_reduce = 0;  // measurement knob (WRONG results): time a step without the split-K reduce

static int current_device() {
    int d = -1;
    return hipGetDevice(&d) == hipSuccess ? d : -1;
}

// the device a stream belongs to: hipStreamGetDevice for a created stream, the current device for
// the null stream.  The queue key must not depend on the calling thread's current device: the
// autograd device thread queues work with the tensor's device current, while the flush may come
// from a thread whose current device is another one.
static int stream_device(hipStream_t st) {
    if (st) {
        hipDevice_t d = -1;
        if (hipStreamGetDevice(st, &d) == hipSuccess && d >= 0) return (int)d;
    }
    return current_device();
}

// the deferral registry (defer.h): one queue per (device, stream)
std::mutex& defer_mutex() {
    static std::mutex m;
    return m;
}

static std::map<std::pair<int, hipStream_t>, DeferQueue>& defer_registry() {
    static std::map<std::pair<int, hipStream_t>, DeferQueue> reg;
    return reg;
}

DeferQueue* defer_queue(hipStream_t st, bool create) {
    auto& reg = defer_registry();
    const auto key = std::make_pair(stream_device(st), st);
    auto it = reg.find(key);
    if (it != reg.end()) return &it->second;
    if (!create) return nullptr;
    DeferQueue& q = reg[key];
    q.stream = st;
    q.device = key.first;
    return &q;
}

// an emptied queue leaves the registry: a stream destroyed after its flush / discard leaves no queue
// behind for a new stream that reuses its handle
void defer_queue_drop(DeferQueue* q) {
    if (q && !q->nred && !q->nadam && !q->parts.n) defer_registry().erase(std::make_pair(q->device, q->stream));
}

// launches of a queue's flush run with the queue's device current (a kernel goes to the stream's
// device), the caller's device restored after
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        const int cur = current_device();
        if (dev >= 0 && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// pending jobs for a launch on stream st of the current device: the stream's split-K reduces, and
// with side_ok (the launch has >= SIDE_MIN free blocks) up to MAX_ADAM of its AdamW jobs, oldest first
RedJobs take_pending_reduces(hipStream_t st, bool side_ok) {
    RedJobs r = {};
    std::lock_guard<std::mutex> lk(defer_mutex());
    DeferQueue* q = defer_queue(st, false);
    if (!q) return r;
    r.n = q->nred;
    for (int i = 0; i < r.n; ++i) r.j[i] = q->red[i];
    q->nred = 0;
    if (side_ok && q->nadam) {
        const int cap = g_adam_per_launch > 0 && g_adam_per_launch < MAX_ADAM ? g_adam_per_launch : MAX_ADAM;
        r.na = q->nadam < cap ? q->nadam : cap;
        for (int i = 0; i < r.na; ++i) r.a[i] = q->adam[i];
        for (int i = r.na; i < q->nadam; ++i) q->adam[i - r.na] = q->adam[i];
        q->nadam -= r.na;
        q->adam_taken += r.na;
    }
#ifdef CG_AB_VARIANTS
    r.adam_batch = g_adam_batch;
#endif
    return r;
}

bool has_pending_reduces(hipStream_t st, bool side_ok) {
    std::lock_guard<std::mutex> lk(defer_mutex());
    const DeferQueue* q = defer_queue(st, false);
    return q && (q->nred || (side_ok && q->nadam));
}

// the stream's pending AdamW jobs: slices of one set of flat buffers with one set of hyperparameters
// (the training step's weight matrices) as ONE segmented launch, anything else job by job
void flush_adam_locked(DeferQueue& q) {
    if (!q.nadam) return;
    const int n = q.nadam;
    q.nadam = 0;
    q.adam_taken += n;   // launched: cg_discard_deferred reports them (cg_flush_deferred resets the count)
    const AdamJob* J = q.adam;
    int b = 0;   // the job with the lowest address is the segments' base
    for (int i = 1; i < n; ++i)
        if (J[i].p < J[b].p) b = i;
    bool one = n > 1 && n <= 64;
    int64_t segs[2 * MAX_ADAM_PENDING];
    for (int i = 0; i < n && one; ++i) {
        const int64_t d = J[i].p - J[b].p;
        one = J[i].g - J[b].g == d && J[i].m - J[b].m == d && J[i].v - J[b].v == d && J[i].pb - J[b].pb == d &&
              J[i].lr == J[b].lr && J[i].beta1 == J[b].beta1 && J[i].beta2 == J[b].beta2 && J[i].eps == J[b].eps &&
              J[i].wd == J[b].wd && J[i].step == J[b].step;
        segs[2 * i] = d;
        segs[2 * i + 1] = 4 * J[i].n4;
    }
    if (one)
        (void)adamw_segments_launch(J[b].p, J[b].g, J[b].m, J[b].v, J[b].pb, segs, n, J[b].lr, J[b].beta1, J[b].beta2,
                                    J[b].eps, J[b].wd, J[b].step, q.stream);
    else
        for (int i = 0; i < n; ++i) (void)adamw_job_launch(J[i], q.stream);
}

// the stream's pending split-K reduces as standalone reduce kernels (cg_flush_deferred, a full queue,
// or an AdamW job whose gradient one of them writes): each one row of n elements through cg_gemm's own
// reduce launch -- the same kernels and summation order as the in-line reduce
void flush_red_locked(DeferQueue& q) {
    const int n = q.nred;
    q.nred = 0;
    for (int i = 0; i < n; ++i) {
        const RedJob& j = q.red[i];
        EpiArgs e{};
        e.kind = CG_EPI_STORE;
        e.dscale = 1.f;
        e.beta = j.beta;
        e.slab_bf16 = j.bf16;
        launch_splitk_reduce(j.ws, j.S, 1, 4 * j.n4, j.out, CG_F32, 4 * j.n4, e, true, q.stream);
    }
}

// Deferred column-sum reduces (the CG_DEFER calls: cg_layernorm_bwd_reduce_ex, cg_reduce_rows_ex,
// cg_head_bwd_ex; the caller keeps every queued job's partials allocated and reads no output before
// cg_flush_deferred on that stream).  The training backward queues its ~20 LayerNorm / bias-gradient
// reduces and the flush launches them as ONE kernel: on one hardware queue each was a ~5 us launch
// for ~1 us of work.  The queue is the stream's DeferQueue (defer.h).
void flush_parts_locked(DeferQueue& q) {
    if (!q.parts.n) return;
    const PartJobs jobs = q.parts;
    q.parts.n = 0;
    launch_reduce_partials_multi(jobs, q.stream);
}

// [p, p + n) of job j's outputs
static bool overlaps(const float* p, int64_t n, const float* q, int64_t m) {
    return p && q && n > 0 && m > 0 && p < q + m && q < p + n;
}
static bool job_outputs_overlap(const PartJob& x, const float* p, int64_t n) {
    return overlaps(x.a, x.S, p, n) || overlaps(x.b, x.S, p, n) || overlaps(x.c, x.N - 2 * x.S, p, n);
}
// an immediate reduce / write into [p, p + n) on stream st: that stream's queued jobs that target it
// go first (caller holds the registry lock)
void flush_parts_touching_locked(DeferQueue* q, const float* p, int64_t n) {
    if (!q) return;
    for (int i = 0; i < q->parts.n; ++i)
        if (job_outputs_overlap(q->parts.j[i], p, n)) {
            flush_parts_locked(*q);
            return;
        }
}

void enqueue_partials(const PartJob& j, hipStream_t st) {
    std::lock_guard<std::mutex> lk(defer_mutex());
    DeferQueue& q = *defer_queue(st, true);
    PartJobs& P = q.parts;
    bool clash = P.n == MAX_PART_JOBS;
    for (int i = 0; i < P.n && !clash; ++i) {
        const PartJob& x = P.j[i];
        clash = job_outputs_overlap(x, j.a, j.S) || job_outputs_overlap(x, j.b, j.S) ||
                job_outputs_overlap(x, j.c, j.N - 2 * j.S);
    }
    if (clash) flush_parts_locked(q);
    if (!P.n) P.start[0] = 0;
    P.j[P.n] = j;
    P.start[P.n + 1] = P.start[P.n] + (int)ceil_div(j.N, 16);
    ++P.n;
}
}  // namespace cg

extern "C" int cg_adamw_defer(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, double lr,
                              double beta1, double beta2, double eps, double weight_decay, const int64_t* step_ptr,
                              void* stream) {
    using namespace cg;
    CG_REQUIRE(p && g && m && v && p_bf16 && step_ptr && n > 0 && n % 4 == 0,
               "cg_adamw_defer: bad arguments (n must be a positive multiple of 4)");
    CG_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0 &&
                   (((uintptr_t)p_bf16) & 7) == 0,
               "cg_adamw_defer: p, g, m, v must be 16-B aligned, p_bf16 8-B aligned");
    hipStream_t st = (hipStream_t)stream;
    {
        std::lock_guard<std::mutex> lk(defer_mutex());
        DeferQueue& q = *defer_queue(st, true);
        DeviceScope ds(q.device);
        // the region's gradient must be final first: a pending split-K reduce or column-sum reduce
        // writing into it goes out now
        for (int i = 0; i < q.nred; ++i)
            if (q.red[i].out < g + n && g < q.red[i].out + 4 * q.red[i].n4) {
                flush_red_locked(q);
                break;
            }
        flush_parts_touching_locked(&q, g, n);
        if (q.nadam == MAX_ADAM_PENDING) flush_adam_locked(q);
        q.adam[q.nadam++] = AdamJob{p, g, m, v, (bf16_t*)p_bf16, n / 4, lr, beta1, beta2, eps, weight_decay, step_ptr};
    }
    CG_LAUNCH_CHECK("cg_adamw_defer");
    return CG_OK;
}

extern "C" int cg_flush_deferred(void* stream) {
    using namespace cg;
    {
        std::lock_guard<std::mutex> lk(defer_mutex());
        DeferQueue* q = defer_queue((hipStream_t)stream, false);
        if (q) {
            DeviceScope ds(q->device);
            flush_red_locked(*q);
            flush_adam_locked(*q);
            flush_parts_locked(*q);
            q->adam_taken = 0;
            defer_queue_drop(q);
        }
    }
    CG_LAUNCH_CHECK("cg_flush_deferred");
    return CG_OK;
}

extern "C" int cg_discard_deferred(void* stream, int* adam_jobs_taken) {
    using namespace cg;
    int taken = 0;
    {
        std::lock_guard<std::mutex> lk(defer_mutex());
        DeferQueue* q = defer_queue((hipStream_t)stream, false);
        if (q) {
            taken = q->adam_taken;
            q->nred = q->nadam = q->parts.n = q->adam_taken = 0;
            defer_queue_drop(q);
        }
    }
    if (adam_jobs_taken) *adam_jobs_taken = taken;
    return CG_OK;
}
