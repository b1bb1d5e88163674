// Launch programs: the native executor of the network passes.
//
// The reference drives its step from Python, one cuDNN call at a time (architectures/deeplab2.py:89-109 expands to ~450
// library ops per pass, train_seg_semisup_mask_mt.py:296-459 issues ~2 k launches per iteration). Round 1 of this build
// kept one Python -> ctypes round trip per convolution (descriptor filled in Python, ~30 us of host time per launch,
// 16 ms per iteration -- close to the 23 ms the GPU needed). Here the host side of a pass is recorded ONCE per input
// shape as a list of launch descriptors over persistent buffers -- convolutions, weight gradients, zero fills, stream
// fork / join points -- and replayed from C++: one call enqueues the whole pass on up to CMS_PROGRAM_MAX_STREAMS HIP
// streams (student || teacher, data gradients || weight gradients), cross-stream order through hipEventRecord /
// hipStreamWaitEvent. Nothing is allocated, nothing synchronises the host; the same call can be stream-captured
// into a hipGraph by the caller since all it does is launch work and record / wait events.
//
// Optional: every k-th convolution launch is bracketed with HIP events on its own stream (bench.py's `roofline`).
// (Cross-stream order through flag words polled on the device instead of events: measured slower in the step and removed --
// docs/DESIGN_HISTORY.md 4.4.)
#include <cstdlib>
#include "common.hpp"
#include <new>
#include <vector>

namespace cms {

enum OpKind { OP_CONV = 0, OP_WGRAD = 1, OP_MEMSET = 2, OP_SYNC = 3, OP_ASPP_GATHER = 4, OP_ASPP_SPREAD = 5, OP_BN = 6, OP_WGRAD_GROUP = 7, OP_CHANNEL_SUM = 8, OP_WGRAD_FINISH = 9 };

struct AsppOp {            // arguments of cms_aspp_gather_fwd / cms_aspp_spread_bwd
    const float* src;      // z / dlogits
    const float* bias;
    void* dst;             // logits / D
    int d_dtype;
    int tap_dy[CMS_CONV_MAX_TAPS], tap_dx[CMS_CONV_MAX_TAPS];
    int n_taps, n, c, zc, h, w;
};

struct Op {
    int kind;
    int stream;        // OP_SYNC: the stream that WAITS
    int from;          // OP_SYNC: the stream whose work is waited for
    int group;         // interleaving key of cms_program_run_pair (bottleneck index)
    int f32;
    cms_conv_desc conv;
    cms_wgrad_desc wg;
    AsppOp aspp;
    cms_bn_op bn;
    void* ptr;
    size_t bytes;
    hipEvent_t ev;     // OP_SYNC
    double flops;
};

struct Timed {
    hipEvent_t e0, e1;
    double flops;
    bool used;
    bool head;         // the ASPP head convolution (fp32 NCHW logits): HBM-bound, accounted separately
};

}  // namespace cms

struct cms_program {
    std::vector<cms::Op> ops;
    int timing_every = 0;
    long conv_seen = 0;
    std::vector<cms::Timed> timed;
    size_t timed_used = 0;
    double acc_ms = 0.0, acc_flops = 0.0;
    long acc_launches = 0;
    long last_head = -1;       // index into `timed` of the head GEMM bracket the next gather op extends
    int last_head_stream = -1;
};

using namespace cms;

static int issue(cms_program* p, Op& o, void* const* streams, int n_streams) {
    CMS_REQUIRE(o.stream >= 0 && o.stream < n_streams, "program: op on stream %d but only %d streams given", o.stream,
                n_streams);
    hipStream_t s = (hipStream_t)streams[o.stream];
    switch (o.kind) {
    case OP_CONV: {
        Timed* t = nullptr;
        const bool head = o.conv.y32 != nullptr;
        if (p->timing_every > 0 && (head || (p->conv_seen++ % p->timing_every) == 0)) {
            if (p->timed_used == p->timed.size()) {
                Timed nt;
                nt.used = false;
                nt.head = false;
                nt.flops = 0.0;
                if (hipEventCreate(&nt.e0) != hipSuccess || hipEventCreate(&nt.e1) != hipSuccess) {
                    set_error("program: hipEventCreate failed");
                    return CMS_ELAUNCH;
                }
                p->timed.push_back(nt);
            }
            t = &p->timed[p->timed_used++];
            t->flops = o.flops;
            t->used = true;
            t->head = head;
            (void)hipEventRecord(t->e0, s);
        }
        const int rc = o.f32 ? cms_conv_igemm_f32(&o.conv, s) : cms_conv_igemm(&o.conv, s);
        if (t) (void)hipEventRecord(t->e1, s);
        p->last_head = (t && head) ? (long)(t - &p->timed[0]) : -1;
        p->last_head_stream = o.stream;
        return rc;
    }
    case OP_ASPP_GATHER: {
        const AsppOp& g = o.aspp;
        const int rc = cms_aspp_gather_fwd(g.src, g.bias, (float*)g.dst, g.tap_dy, g.tap_dx, g.n_taps, g.n, g.c, g.zc, g.h,
                                           g.w, s);
        // the head = GEMM + gather: move the closing event of the GEMM's bracket behind the gather
        if (p->last_head >= 0 && p->last_head_stream == o.stream) (void)hipEventRecord(p->timed[p->last_head].e1, s);
        p->last_head = -1;
        return rc;
    }
    case OP_ASPP_SPREAD: {
        const AsppOp& g = o.aspp;
        return cms_aspp_spread_bwd(g.src, g.dst, g.d_dtype, g.tap_dy, g.tap_dx, g.n_taps, g.n, g.c, g.zc, g.h, g.w, s);
    }
    case OP_WGRAD:
        return o.f32 ? cms_conv_wgrad_f32(&o.wg, s) : cms_conv_wgrad(&o.wg, s);
    case OP_WGRAD_GROUP:        // ptr = the device-resident item table, bytes = items, from = grid size, f32 = kind
        return cms_conv_wgrad_group_run(o.ptr, (int)o.bytes, o.from, o.f32, s);
    case OP_CHANNEL_SUM:        // ptr = src, bytes = rows, from = channels, f32 = dtype code, aspp.dst = the fp32 sums
        return cms_channel_sum(o.ptr, o.f32, o.bytes, o.from, (float*)o.aspp.dst, s);
    case OP_WGRAD_FINISH:       // ptr = the device-resident item table, bytes = items, from = grid size
        return cms_wgrad_finish_run(o.ptr, (int)o.bytes, o.from, s);
    case OP_BN: return cms_bn_run(&o.bn, s);
    case OP_MEMSET:
        if (hipMemsetAsync(o.ptr, 0, o.bytes, s) != hipSuccess) {
            set_error("program: hipMemsetAsync failed");
            return CMS_ELAUNCH;
        }
        return CMS_OK;
    case OP_SYNC: {
        CMS_REQUIRE(o.from >= 0 && o.from < n_streams, "program: sync from stream %d but only %d streams given", o.from,
                    n_streams);
        if (streams[o.from] == streams[o.stream]) return CMS_OK;      // same stream: already ordered
        if (hipEventRecord(o.ev, (hipStream_t)streams[o.from]) != hipSuccess ||
            hipStreamWaitEvent(s, o.ev, 0) != hipSuccess) {
            set_error("program: event record / wait failed");
            return CMS_ELAUNCH;
        }
        return CMS_OK;
    }
    }
    set_error("program: unknown op kind %d", o.kind);
    return CMS_EINVAL;
}

extern "C" int cms_program_create(cms_program** out) {
    CMS_REQUIRE(out != nullptr, "program_create: NULL out pointer");
    *out = new (std::nothrow) cms_program();
    CMS_REQUIRE(*out != nullptr, "program_create: out of host memory");
    return CMS_OK;
}

extern "C" int cms_program_destroy(cms_program* p) {
    if (!p) return CMS_OK;
    for (auto& o : p->ops)
        if (o.kind == OP_SYNC && o.ev) (void)hipEventDestroy(o.ev);
    for (auto& t : p->timed) {
        (void)hipEventDestroy(t.e0);
        (void)hipEventDestroy(t.e1);
    }
    delete p;
    return CMS_OK;
}

static int push(cms_program* p, const Op& o) {
    p->ops.push_back(o);
    return (int)p->ops.size() - 1;
}

extern "C" int cms_program_add_conv(cms_program* p, const cms_conv_desc* d, int f32, int stream_idx, int group) {
    CMS_REQUIRE(p && d, "program_add_conv: NULL pointer");
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_conv: stream index %d", stream_idx);
    Op o = {};
    o.kind = OP_CONV; o.stream = stream_idx; o.group = group; o.f32 = f32 ? 1 : 0;
    o.conv = *d;
    o.flops = 2.0 * (double)d->n * d->ho * d->wo * (double)d->cout * d->cin * d->ntaps;
    return push(p, o);
}

extern "C" int cms_program_add_wgrad(cms_program* p, const cms_wgrad_desc* d, int f32, int stream_idx, int group) {
    CMS_REQUIRE(p && d, "program_add_wgrad: NULL pointer");
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_wgrad: stream index %d", stream_idx);
    Op o = {};
    o.kind = OP_WGRAD; o.stream = stream_idx; o.group = group; o.f32 = f32 ? 1 : 0;
    o.wg = *d;
    o.flops = 2.0 * (double)d->n * d->ho * d->wo * (double)d->cout * d->cin * d->ntaps;
    return push(p, o);
}

extern "C" int cms_program_add_wgrad_group(cms_program* p, const void* table_dev, int n_items, int total_blocks, int kind, int stream_idx,
                                           int group) {
    CMS_REQUIRE(p && table_dev && n_items > 0 && total_blocks > 0 && (kind == 1 || kind == 2), "program_add_wgrad_group: bad arguments");
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_wgrad_group: stream index %d", stream_idx);
    Op o = {};
    o.kind = OP_WGRAD_GROUP; o.stream = stream_idx; o.group = group;
    o.ptr = const_cast<void*>(table_dev); o.bytes = (size_t)n_items; o.from = total_blocks; o.f32 = kind;
    return push(p, o);
}

extern "C" int cms_program_add_channel_sum(cms_program* p, const void* src, int dtype, size_t rows, int channels, float* dst,
                                           int stream_idx, int group) {
    CMS_REQUIRE(p && src && dst && rows > 0 && channels > 0 && channels % 64 == 0, "program_add_channel_sum: bad arguments");
    CMS_REQUIRE(dtype == CMS_F32 || dtype == CMS_BF16, "program_add_channel_sum: bad dtype");
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_channel_sum: stream index %d", stream_idx);
    Op o = {};
    o.kind = OP_CHANNEL_SUM; o.stream = stream_idx; o.group = group;
    o.ptr = const_cast<void*>(src); o.bytes = rows; o.from = channels; o.f32 = dtype; o.aspp.dst = dst;
    return push(p, o);
}

extern "C" int cms_program_add_wgrad_finish(cms_program* p, const void* items_dev, int n_items, int total_blocks, int stream_idx,
                                            int group) {
    CMS_REQUIRE(p && items_dev && n_items > 0 && total_blocks > 0, "program_add_wgrad_finish: bad arguments");
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_wgrad_finish: stream index %d", stream_idx);
    Op o = {};
    o.kind = OP_WGRAD_FINISH; o.stream = stream_idx; o.group = group;
    o.ptr = const_cast<void*>(items_dev); o.bytes = (size_t)n_items; o.from = total_blocks;
    return push(p, o);
}

extern "C" int cms_program_add_memset(cms_program* p, void* ptr, size_t bytes, int stream_idx, int group) {
    CMS_REQUIRE(p && ptr && bytes > 0, "program_add_memset: NULL pointer / empty range");
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_memset: stream index %d", stream_idx);
    Op o = {};
    o.kind = OP_MEMSET; o.stream = stream_idx; o.group = group; o.ptr = ptr; o.bytes = bytes;
    return push(p, o);
}

extern "C" int cms_program_add_sync(cms_program* p, int from_stream, int to_stream, int group) {
    CMS_REQUIRE(p, "program_add_sync: NULL program");
    CMS_REQUIRE(from_stream >= 0 && from_stream < CMS_PROGRAM_MAX_STREAMS && to_stream >= 0 &&
                    to_stream < CMS_PROGRAM_MAX_STREAMS, "program_add_sync: stream indices %d -> %d", from_stream, to_stream);
    Op o = {};
    o.kind = OP_SYNC; o.stream = to_stream; o.from = from_stream; o.group = group;
    if (hipEventCreateWithFlags(&o.ev, hipEventDisableTiming) != hipSuccess) {
        set_error("program_add_sync: hipEventCreate failed");
        return CMS_ELAUNCH;
    }
    return push(p, o);
}

static int add_aspp(cms_program* p, int kind, const float* src, const float* bias, void* dst, int d_dtype, const int* dy,
                    const int* dx, int n_taps, int n, int c, int zc, int h, int w, int stream_idx, int group) {
    CMS_REQUIRE(p && src && dst && dy && dx, "program_add_aspp: NULL pointer");
    CMS_REQUIRE(n_taps > 0 && n_taps <= CMS_CONV_MAX_TAPS, "program_add_aspp: 1..%d taps", CMS_CONV_MAX_TAPS);
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_aspp: stream index %d", stream_idx);
    Op o = {};
    o.kind = kind; o.stream = stream_idx; o.group = group;
    o.aspp.src = src; o.aspp.bias = bias; o.aspp.dst = dst; o.aspp.d_dtype = d_dtype;
    for (int i = 0; i < n_taps; ++i) { o.aspp.tap_dy[i] = dy[i]; o.aspp.tap_dx[i] = dx[i]; }
    o.aspp.n_taps = n_taps; o.aspp.n = n; o.aspp.c = c; o.aspp.zc = zc; o.aspp.h = h; o.aspp.w = w;
    return push(p, o);
}

extern "C" int cms_program_add_aspp_gather(cms_program* p, const float* z, const float* bias, float* logits, const int* tap_dy,
                                           const int* tap_dx, int n_taps, int n, int c, int zc, int h, int w, int stream_idx,
                                           int group) {
    return add_aspp(p, OP_ASPP_GATHER, z, bias, logits, CMS_F32, tap_dy, tap_dx, n_taps, n, c, zc, h, w, stream_idx, group);
}

extern "C" int cms_program_add_aspp_spread(cms_program* p, const float* dlogits, void* d_nhwc, int d_dtype, const int* tap_dy,
                                           const int* tap_dx, int n_taps, int n, int c, int zc, int h, int w, int stream_idx,
                                           int group) {
    return add_aspp(p, OP_ASPP_SPREAD, dlogits, nullptr, d_nhwc, d_dtype, tap_dy, tap_dx, n_taps, n, c, zc, h, w, stream_idx,
                    group);
}

extern "C" int cms_program_add_bn(cms_program* p, const cms_bn_op* op, int stream_idx, int group) {
    CMS_REQUIRE(p && op, "program_add_bn: NULL pointer");
    CMS_REQUIRE(op->what >= CMS_BN_REDUCE && op->what <= CMS_BN_BWD_SUMS_TILES, "program_add_bn: unknown op %d", op->what);
    CMS_REQUIRE((op->what != CMS_BN_FINALIZE_TILES && op->what != CMS_BN_BWD_SUMS_TILES) || (op->ws && op->tile_rows > 0),
                "program_add_bn: finalize_tiles / sums_tiles need the tile sums (ws) and the tile rows");
    CMS_REQUIRE(op->what != CMS_BN_BWD_SUMS_TILES || op->sums, "program_add_bn: sums_tiles writes `sums`");
    CMS_REQUIRE(op->groups <= 1 || op->ws || (op->what != CMS_BN_REDUCE && op->what != CMS_BN_REDUCE_BWD),
                "program_add_bn: grouped reductions need a workspace");
    CMS_REQUIRE(op->what != CMS_BN_REDUCE_BWD || !op->mask_bits || op->ws,
                "program_add_bn: the backward reduction reads mask bits on the workspace kernels only");
    CMS_REQUIRE(stream_idx >= 0 && stream_idx < CMS_PROGRAM_MAX_STREAMS, "program_add_bn: stream index %d", stream_idx);
    Op o = {};
    o.kind = OP_BN; o.stream = stream_idx; o.group = group;
    o.bn = *op;
    return push(p, o);
}

extern "C" int cms_program_size(const cms_program* p) { return p ? (int)p->ops.size() : 0; }

extern "C" int cms_program_run(cms_program* p, int first, int last, void* const* streams, int n_streams) {
    CMS_REQUIRE(p && streams && n_streams > 0, "program_run: NULL program / streams");
    const int n = (int)p->ops.size();
    if (last < 0 || last > n) last = n;
    CMS_REQUIRE(first >= 0 && first <= last, "program_run: bad range [%d, %d) of %d ops", first, last, n);
    for (int i = first; i < last; ++i) {
        const int rc = issue(p, p->ops[i], streams, n_streams);
        if (rc != CMS_OK) return rc;
    }
    return CMS_OK;
}

// Two programs issued interleaved, group by group (ops of `a` with group g, then ops of `b` with group g, ...): keeps
// two kernels in flight for the whole pass when the programs run on different streams (student || teacher).
extern "C" int cms_program_run_pair(cms_program* a, void* const* streams_a, int na, cms_program* b,
                                    void* const* streams_b, int nb) {
    CMS_REQUIRE(a && b && streams_a && streams_b && na > 0 && nb > 0, "program_run_pair: NULL program / streams");
    size_t ia = 0, ib = 0;
    const size_t ea = a->ops.size(), eb = b->ops.size();
    // (the two passes forced into phase at group boundaries: measured, not adopted -- DESIGN 4.1 round 6)
    while (ia < ea || ib < eb) {
        // next group = the smaller of the two heads' groups (groups are recorded in non-decreasing order)
        const int ga = ia < ea ? a->ops[ia].group : 0x7fffffff;
        const int gb = ib < eb ? b->ops[ib].group : 0x7fffffff;
        const int g = ga < gb ? ga : gb;
        while (ia < ea && a->ops[ia].group <= g) {
            const int rc = issue(a, a->ops[ia++], streams_a, na);
            if (rc != CMS_OK) return rc;
        }
        while (ib < eb && b->ops[ib].group <= g) {
            const int rc = issue(b, b->ops[ib++], streams_b, nb);
            if (rc != CMS_OK) return rc;
        }
    }
    return CMS_OK;
}

extern "C" int cms_program_set_timing(cms_program* p, int every_k) {
    CMS_REQUIRE(p, "program_set_timing: NULL program");
    p->timing_every = every_k > 0 ? every_k : 0;
    return CMS_OK;
}

// Sums the event-bracketed convolution launches since the last call (waits for them to finish) and resets.
extern "C" int cms_program_read_timing(cms_program* p, double* sum_ms, double* sum_flops, long* launches,
                                       double* head_ms, long* head_launches) {
    CMS_REQUIRE(p, "program_read_timing: NULL program");
    double ms = 0.0, fl = 0.0, hms = 0.0;
    long n = 0, hn = 0;
    for (size_t i = 0; i < p->timed_used; ++i) {
        Timed& t = p->timed[i];
        if (!t.used) continue;
        float dt = 0.0f;
        if (hipEventSynchronize(t.e1) != hipSuccess || hipEventElapsedTime(&dt, t.e0, t.e1) != hipSuccess) {
            set_error("program_read_timing: event query failed");
            return CMS_ELAUNCH;
        }
        if (t.head) {
            hms += dt;
            ++hn;
        } else {
            ms += dt;
            fl += t.flops;
            ++n;
        }
        t.used = false;
    }
    p->timed_used = 0;
    if (sum_ms) *sum_ms = ms;
    if (sum_flops) *sum_flops = fl;
    if (launches) *launches = n;
    if (head_ms) *head_ms = hms;
    if (head_launches) *head_launches = hn;
    return CMS_OK;
}
