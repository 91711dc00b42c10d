// charpt deferred work (include/charpt.h "Deferred work"): the split-K reduces a cg_gemm call with
// CG_GEMM_DEFER_REDUCE leaves pending, the AdamW updates of cg_adamw_defer and the column-sum reduces
// of the CG_DEFER calls.  Every queue belongs to ONE stream of one device: only a persistent GEMM
// launch on that stream takes its jobs, cg_flush_deferred(stream) launches the rest, and a mutex
// guards the registry -- host threads that each drive their own stream share no state.
#pragma once
#include <mutex>

#include "gemm_common.h"

namespace cg {

// one queued column-sum reduce (reduce_partials_deferrable): outputs a / b / c, S columns each
struct PartJob {
    const float* part;
    int64_t K, N, S;
    float *a, *b, *c;
    int acc, acc_c;
};
constexpr int MAX_PART_JOBS = 24;
struct PartJobs {
    int n;
    int start[MAX_PART_JOBS + 1];   // first block of job q; start[n] = the grid
    PartJob j[MAX_PART_JOBS];
};

constexpr int MAX_ADAM_PENDING = 64;

struct DeferQueue {
    hipStream_t stream = nullptr;
    int device = -1;
    RedJob red[MAX_RED];
    int nred = 0;
    AdamJob adam[MAX_ADAM_PENDING];
    int nadam = 0;
    int adam_taken = 0;   // AdamW jobs GEMM launches took since the last flush / discard
    PartJobs parts = {};
};

// the registry lock; every function below expects the caller to hold it
std::mutex& defer_mutex();
// the queue of stream st (keyed by the stream's own device); nullptr when it has none and !create
DeferQueue* defer_queue(hipStream_t st, bool create);
// remove an emptied queue from the registry (q is invalid afterwards)
void defer_queue_drop(DeferQueue* q);
// queued column-sum reduces whose outputs overlap [p, p + n) go out now
void flush_parts_touching_locked(DeferQueue* q, const float* p, int64_t n);
// launch (on the queue's stream) and clear one kind of job
void flush_red_locked(DeferQueue& q);
void flush_adam_locked(DeferQueue& q);
void flush_parts_locked(DeferQueue& q);
// queue one column-sum reduce on stream st (takes the lock itself)
void enqueue_partials(const PartJob& j, hipStream_t st);

// defer.hip holds host code only; the kernels its flushes launch:
void launch_reduce_partials_multi(const PartJobs& jobs, hipStream_t st);   // reduce.hip
int adamw_job_launch(const AdamJob& j, hipStream_t st);                    // adamw.hip
int adamw_segments_launch(float* p, const float* g, float* m, float* v, bf16_t* pb, const int64_t* segs, int nseg,
                          double lr, double beta1, double beta2, double eps, double wd, const int64_t* step,
                          hipStream_t st);                                 // adamw.hip

// cg_set_tuning knobs (defer.hip; g_red_side is with take_pending_reduces in gemm_common.h)
extern int g_adam_per_launch;      // AdamW jobs one launch's free blocks take (0 = MAX_ADAM)
extern int g_adam_batch;           // A/B build only: the side blocks' AdamW chunks in flight per thread
extern int g_skip_splitk_reduce;   // measurement knob (WRONG results): time a step without the split-K reduce

}  // namespace cg
