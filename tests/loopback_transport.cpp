// loopback_transport.cpp -- a test-only vr_transport (include/vrhip.h) that connects `world` compositors of ONE process
// on ONE GPU, so that vr_compositor_composite's world > 1 exchange runs without RCCL (two RCCL ranks cannot share a
// device).  Each rank is driven from its own host thread.  Plain C++ on the HIP runtime API, built by the tests with g++:
//
//   g++ -std=c++14 -O2 -Wall -Werror -fPIC -shared -pthread -D__HIP_PLATFORM_AMD__ -I$ROCM/include
//       loopback_transport.cpp -L$ROCM/lib -lamdhip64 -Wl,-rpath,$ROCM/lib -o libloopback.so
//
// Semantics: NCCL's grouped point-to-point model, and nothing stronger.
//  - send / recv only inside group_start .. group_end; every operation of one rank's group uses one stream.
//  - group_end records an event on the rank's stream (its sends' data is ready there), publishes the rank's queue and
//    waits at a barrier of all ranks, bounded by the timeout given at creation: on expiry it returns an error.
//  - the k-th send from p to r matches the k-th recv on r from p; a count mismatch or an unmatched operation fails the
//    group on every rank (the check runs on the published queues of all ranks, so every rank reaches the same verdict)
//    and nothing is copied.
//  - a recv becomes hipStreamWaitEvent(own stream, sender's event) + hipMemcpyAsync device to device on its own
//    stream; after a second barrier every sender's stream waits for the completion events of the ranks it sent to, so
//    that work the sender queues later may overwrite what it sent.
//  - no host or device synchronisation anywhere: a missing dependency on the caller's stream shows as a wrong frame.
//  - a group in which a call failed (lb_fail_at) is abandoned: its group_end closes it and returns an error without
//    joining the barrier, so the peers see the bounded wait expire.  After an expiry every later wait fails at once.
// Every call is logged (group index of the rank, rank, peer, kind, count) for the tests to read.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace {

enum Kind { GROUP_START = 0, GROUP_END = 1, SEND = 2, RECV = 3 };

struct Op {
    int kind, peer;
    const float *src;
    float *dst;
    int64_t count;
};

struct Entry {
    int group, rank, peer, kind;
    int64_t count;
};

struct Inject {
    int group, rank, call;
    bool fail;
    int64_t delta;   // added to the count the fake records (fail == false)
};

struct Fake;

struct Rank {
    Fake *f = nullptr;
    int rank = 0;
    bool inGroup = false, abandoned = false, haveStream = false;
    int group = -1, calls = 0;
    hipStream_t stream = nullptr;
    std::vector<Op> ops;
    hipEvent_t ready = nullptr, done = nullptr;
};

struct Fake {
    int world = 0;
    double timeout = 30.0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    bool broken = false;
    std::vector<Rank> ranks;
    std::vector<Entry> log;
    std::vector<Inject> injects;
    std::string errors;
};

typedef int32_t (*GroupFn)(void *);
typedef int32_t (*SendFn)(void *, const float *, int64_t, int32_t, void *);
typedef int32_t (*RecvFn)(void *, float *, int64_t, int32_t, void *);
struct Table {   // the layout of vr_transport
    GroupFn group_start, group_end;
    SendFn send;
    RecvFn recv;
};

__attribute__((format(printf, 2, 3))) void note(Fake &f, const char *fmt, ...)
{   // with f.m held
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (!f.errors.empty()) f.errors += "; ";
    f.errors += buf;
}

bool barrier(Fake &f, std::unique_lock<std::mutex> &lk, int rank)
{   // with f.m held; false when the wait expired (now or before)
    if (f.broken) return false;
    const uint64_t gen = f.generation;
    if (++f.arrived == f.world) {
        f.arrived = 0;
        ++f.generation;
        f.cv.notify_all();
        return true;
    }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(f.timeout);
    while (f.generation == gen && !f.broken)
        if (f.cv.wait_until(lk, deadline) == std::cv_status::timeout && f.generation == gen && !f.broken) {
            f.broken = true;
            note(f, "rank %d: barrier timed out after %.3f s with %d of %d ranks there", rank, f.timeout, f.arrived, f.world);
            f.cv.notify_all();
        }
    return f.generation != gen;
}

int32_t lb_group_start(void *ctx)
{
    Rank &r = *(Rank *)ctx;
    Fake &f = *r.f;
    std::unique_lock<std::mutex> lk(f.m);
    f.log.push_back({r.group + 1, r.rank, -1, GROUP_START, 0});
    if (r.inGroup) { note(f, "rank %d: group_start inside group %d", r.rank, r.group); return 1; }
    ++r.group;
    r.inGroup = true; r.abandoned = false; r.haveStream = false; r.calls = 0;
    r.ops.clear();
    return 0;
}

int32_t queue_op(Rank &r, int kind, const float *src, float *dst, int64_t count, int32_t peer, void *stream)
{
    Fake &f = *r.f;
    std::unique_lock<std::mutex> lk(f.m);
    const int call = r.calls++;
    int64_t recorded = count;
    bool fail = false;
    for (const Inject &in : f.injects)
        if (r.inGroup && in.group == r.group && in.rank == r.rank && in.call == call) {
            if (in.fail) fail = true;
            else recorded += in.delta;
        }
    f.log.push_back({r.inGroup ? r.group : -1, r.rank, peer, kind, recorded});
    const char *what = kind == SEND ? "send" : "recv";
    if (!r.inGroup) { note(f, "rank %d: %s (peer %d, count %lld) outside a group", r.rank, what, peer, (long long)count); return 1; }
    if (fail) { r.abandoned = true; note(f, "rank %d: injected failure of %s %d in group %d", r.rank, what, call, r.group); return 1; }
    if (peer < 0 || peer >= f.world || peer == r.rank || count < 0 || (count > 0 && !(kind == SEND ? (const void *)src : (const void *)dst))) {
        r.abandoned = true;
        note(f, "rank %d: bad %s (peer %d, count %lld)", r.rank, what, peer, (long long)count);
        return 1;
    }
    if (r.haveStream && (hipStream_t)stream != r.stream) {
        r.abandoned = true;
        note(f, "rank %d: %s %d of group %d uses a second stream", r.rank, what, call, r.group);
        return 1;
    }
    r.stream = (hipStream_t)stream;
    r.haveStream = true;
    r.ops.push_back({kind, peer, src, dst, recorded});
    return 0;
}

int32_t lb_send(void *ctx, const float *buf, int64_t count, int32_t peer, void *stream)
{
    return queue_op(*(Rank *)ctx, SEND, buf, nullptr, count, peer, stream);
}

int32_t lb_recv(void *ctx, float *buf, int64_t count, int32_t peer, void *stream)
{
    return queue_op(*(Rank *)ctx, RECV, nullptr, buf, count, peer, stream);
}

// the j-th operation of `kind` between (a -> peer b) in a's queue, or null
const Op *nth(const Rank &a, int kind, int b, int j)
{
    for (const Op &o : a.ops)
        if (o.kind == kind && o.peer == b && j-- == 0) return &o;
    return nullptr;
}
int count_of(const Rank &a, int kind, int b)
{
    int n = 0;
    for (const Op &o : a.ops) n += o.kind == kind && o.peer == b;
    return n;
}

int32_t lb_group_end(void *ctx)
{
    Rank &r = *(Rank *)ctx;
    Fake &f = *r.f;
    std::unique_lock<std::mutex> lk(f.m);
    f.log.push_back({r.group, r.rank, -1, GROUP_END, 0});
    if (!r.inGroup) { note(f, "rank %d: group_end outside a group", r.rank); return 1; }
    r.inGroup = false;
    if (r.abandoned) return 1;
    // my sends' data is ready at this point of my stream
    if (r.haveStream && hipEventRecord(r.ready, r.stream) != hipSuccess) { note(f, "rank %d: hipEventRecord failed", r.rank); return 1; }
    if (!barrier(f, lk, r.rank)) return 1;
    // every rank's queue is published: match them all (the same verdict on every rank)
    bool ok = true;
    for (int p = 0; p < f.world; ++p)
        for (int q = 0; q < f.world; ++q) {
            if (p == q) continue;
            const int ns = count_of(f.ranks[p], SEND, q), nr = count_of(f.ranks[q], RECV, p);
            if (ns != nr) {
                ok = false;
                if (r.rank == 0) note(f, "group %d: %d sends from rank %d to rank %d, %d recvs on rank %d from rank %d", r.group, ns, p, q, nr, q, p);
                continue;
            }
            for (int j = 0; j < ns; ++j) {
                const Op *s = nth(f.ranks[p], SEND, q, j), *v = nth(f.ranks[q], RECV, p, j);
                if (s->count != v->count) {
                    ok = false;
                    if (r.rank == 0) note(f, "group %d: rank %d sends %lld floats to rank %d, which receives %lld", r.group, p, (long long)s->count, q, (long long)v->count);
                }
            }
        }
    if (ok) {
        std::vector<int> seen(f.world, 0);
        for (const Op &o : r.ops) {
            if (o.kind != RECV) continue;
            const Op *s = nth(f.ranks[o.peer], SEND, r.rank, seen[o.peer]++);
            if (hipStreamWaitEvent(r.stream, f.ranks[o.peer].ready, 0) != hipSuccess ||
                (o.count && hipMemcpyAsync(o.dst, s->src, (size_t)o.count * sizeof(float), hipMemcpyDeviceToDevice, r.stream) != hipSuccess)) {
                note(f, "rank %d: copy from rank %d failed", r.rank, o.peer);
                ok = false;
            }
        }
        if (r.haveStream && hipEventRecord(r.done, r.stream) != hipSuccess) ok = false;
    }
    // every receiver has queued its copies and recorded `done` before a sender waits for it
    if (!barrier(f, lk, r.rank)) return 1;
    if (!ok) return 1;
    for (int q = 0; q < f.world; ++q)
        if (q != r.rank && count_of(r, SEND, q) > 0 && hipStreamWaitEvent(r.stream, f.ranks[q].done, 0) != hipSuccess) {
            note(f, "rank %d: wait for rank %d failed", r.rank, q);
            return 1;
        }
    return 0;
}

const Table kTable = {lb_group_start, lb_group_end, lb_send, lb_recv};

} // namespace

extern "C" {

// a fake for `world` ranks; group_end's waits give up after timeout_s seconds (<= 0: 30 s).  Null on failure.
void *lb_create(int32_t world, double timeout_s)
{
    if (world < 1) return nullptr;
    Fake *f = new Fake();
    f->world = world;
    f->timeout = timeout_s > 0 ? timeout_s : 30.0;
    f->ranks.resize(world);
    for (int i = 0; i < world; ++i) {
        Rank &r = f->ranks[i];
        r.f = f;
        r.rank = i;
        if (hipEventCreateWithFlags(&r.ready, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&r.done, hipEventDisableTiming) != hipSuccess) {
            for (Rank &q : f->ranks) { if (q.ready) hipEventDestroy(q.ready); if (q.done) hipEventDestroy(q.done); }
            delete f;
            return nullptr;
        }
    }
    return f;
}

void lb_destroy(void *fake)
{
    Fake *f = (Fake *)fake;
    if (!f) return;
    for (Rank &r : f->ranks) { hipEventDestroy(r.ready); hipEventDestroy(r.done); }
    delete f;
}

// the ctx to give vr_compositor_create_with_transport for `rank`
void *lb_rank_ctx(void *fake, int32_t rank)
{
    Fake *f = (Fake *)fake;
    return f && rank >= 0 && rank < f->world ? (void *)&f->ranks[rank] : nullptr;
}

// the vr_transport table of the fake
const void *lb_transport(void) { return &kTable; }

// the `call`-th send / recv (from 0) of `rank`'s group `group` (from 0) fails; the compositor must still close the group
void lb_fail_at(void *fake, int32_t group, int32_t rank, int32_t call)
{
    Fake *f = (Fake *)fake;
    std::lock_guard<std::mutex> lk(f->m);
    f->injects.push_back({group, rank, call, true, 0});
}

// the `call`-th send / recv of `rank`'s group `group` is recorded with `delta` floats more than the caller asked for
void lb_count_delta(void *fake, int32_t group, int32_t rank, int32_t call, int64_t delta)
{
    Fake *f = (Fake *)fake;
    std::lock_guard<std::mutex> lk(f->m);
    f->injects.push_back({group, rank, call, false, delta});
}

int32_t lb_log_size(void *fake)
{
    Fake *f = (Fake *)fake;
    std::lock_guard<std::mutex> lk(f->m);
    return (int32_t)f->log.size();
}

// entry i: out[0..4] = group, rank, peer (-1 for group_start / group_end), kind (0 group_start, 1 group_end, 2 send,
// 3 recv), count in floats.  0 on success.
int32_t lb_log_entry(void *fake, int32_t i, int64_t out[5])
{
    Fake *f = (Fake *)fake;
    std::lock_guard<std::mutex> lk(f->m);
    if (i < 0 || i >= (int32_t)f->log.size()) return 1;
    const Entry &e = f->log[i];
    out[0] = e.group; out[1] = e.rank; out[2] = e.peer; out[3] = e.kind; out[4] = e.count;
    return 0;
}

void lb_log_clear(void *fake)
{
    Fake *f = (Fake *)fake;
    std::lock_guard<std::mutex> lk(f->m);
    f->log.clear();
}

// the errors so far, "; "-separated, NUL-terminated into buf[n]; returns the full length
int32_t lb_errors(void *fake, char *buf, int32_t n)
{
    Fake *f = (Fake *)fake;
    std::lock_guard<std::mutex> lk(f->m);
    if (buf && n > 0) {
        strncpy(buf, f->errors.c_str(), (size_t)n - 1);
        buf[n - 1] = 0;
    }
    return (int32_t)f->errors.size();
}

} // extern "C"
