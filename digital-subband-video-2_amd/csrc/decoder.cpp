// decoder.cpp -- host frame controller of the decoder (C ABI section 3 of include/dsv2_hip.h).
//
// Restates the serial parsing of reference src/dsv_decoder.c (packet header :22, metadata :52,
// stability blocks :177, intra metadata :202, motion data :82, picture packet :394) and drives
// the device pipeline: symbol scatter + dequantisation -> inverse SBT -> intra filter, or
// motion-compensated prediction + reconstruction + in-loop filters -> border extension of
// reference pictures.  Entropy *parsing* is serial adaptive-state work and stays on the host.
#include <sched.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <vector>

#include "batch.h"
#include "codec.h"
#include "dec_delivery.h"
#include "dec_parse.h"
#include "dec_parse_dev.h"
#include "overlay.h"

using namespace dsv2;
using namespace dsv2::decparse;
using namespace dsv2::delivery;

namespace {

struct DecImpl {
    CodecDev dev;
    bool ready = false;
    int cur = 0;
    bool have_ref = false;
    SideBufs side;                  // per-block flag bytes and vectors as parsed (dec_parse.h)
    std::vector<DSV_MV> &mvs = side.mvs;
    std::vector<uint8_t> &blockdata = side.blockdata;
    std::vector<uint32_t> pos;
    std::vector<int32_t> val;
    bool out420p = false; // deliver every picture as 4:2:0 (the CLI's -out420p, util.c:79-153, done by the GPU on the way out)
    bool postsharp = false; // dsv_post_process on the luma of every picture handed out (the CLI's -postsharp, dsv_main.c:1084-1089)
    // RGB delivery of a drawn-on or sharpened picture: there is no delivered luma plane for the overlay and the sharpening to act on,
    // so the luma is staged here (w x h, 16-byte aligned origin and stride) and converted from here; made on first use
    DPlane rgb_luma = {nullptr, 0, 0, 0};
    const DPlane &staged_luma()
    {
        if (!rgb_luma.data) {
            const int stride = (dev.w + 15) & ~15;
            HIPCHK(dev_alloc((void **) &rgb_luma.data, (size_t) stride * (size_t) dev.h));
            rgb_luma.stride = stride, rgb_luma.w = dev.w, rgb_luma.h = dev.h;
        }
        return rgb_luma;
    }
    // Scaled delivery (DSV2HIP_SCALE_*) and sized delivery into a semiplanar or an RGB surface: the reduced planes that k_egress_uv /
    // k_egress_rgb then read are staged here.  Sized for half size -- a quarter of a picture -- and laid out once with its strides; a
    // quarter- or eighth-size picture uses the top left of the same planes.  A sized picture can be as large as the picture itself:
    // the first one (full) replaces the staging by one of the planes' own sizes, which serves every later delivery and is kept
    // (four times the half-size layout's bytes) until destroy_dev.  The rounds of a
    // decoder follow one another with the stream drained in between, so nothing reads the staging that is released.  16-byte aligned
    // origins and strides, so rows are readable (and, by the wide forms of the reduction and the resampling, writable) up to the next
    // multiple of 16 bytes; made on first use
    DPlane scaled[3] = {{nullptr, 0, 0, 0}, {nullptr, 0, 0, 0}, {nullptr, 0, 0, 0}};
    bool scaled_full = false;
    const DPlane *staged_scaled(bool full)
    {
        if (scaled[0].data && full && !scaled_full) {
            dev_release(scaled[0].data);
            scaled[0].data = nullptr;
        }
        if (!scaled[0].data) {
            scaled_full = full;
            size_t off[3], total = 0;
            for (int c = 0; c < 3; c++) {
                const DPlane &p = dev.pics[0].recon.p[c];
                scaled[c].w = full ? p.w : (p.w + 1) >> 1, scaled[c].h = full ? p.h : (p.h + 1) >> 1;
                scaled[c].stride = (scaled[c].w + 15) & ~15;
                off[c] = total;
                total += (size_t) scaled[c].stride * (size_t) scaled[c].h;
            }
            uint8_t *base = nullptr;
            HIPCHK(dev_alloc((void **) &base, total));
            for (int c = 0; c < 3; c++) {
                scaled[c].data = base + off[c];
            }
        }
        return scaled;
    }
    void destroy_dev() // the device instance and what was sized by its geometry
    {
        dev.destroy();
        dev_release(rgb_luma.data);
        rgb_luma = DPlane{nullptr, 0, 0, 0};
        dev_release(scaled[0].data);
        scaled[0].data = nullptr;
    }
};

// ---- lockstep batch engine ------------------------------------------------------------------------
// One step decodes ONE packet on each of n decoder instances (dsv_dec is the n = 1 case):
//   A host   (one pool task per stream) packet header, metadata, per-block side information and the
//            serial entropy parse of the three planes into (position, value) symbol lists
//   B device every picture of the step in one set of launches over job tables: zero + scatter/dequantise
//            the coefficient planes, inverse transform, intra filter or motion-compensated
//            reconstruction + in-loop filters, border extension, picture to pinned host memory or (dsv2hip_dec_batch_device,
//            dsv2hip_dec_batch_surface) into the caller's device planes; on that way out: 4:2:0 conversion, chroma interleave,
//            draw_info overlay, postsharp
//   C host   (one pool task per stream) output frame, reference bookkeeping
// Pictures of a step whose geometry differs from the first one are decoded in a second round.
struct DecJob {
    DSV_DECODER *d;
    DSV_BUF *buf;
    DSV_FRAME **out;
    DSV_FNUM *fn;
    int ret = DSV_DEC_OK;
    bool pic = false; // a picture that takes part in the device phase
    DecImpl *im = nullptr;
    int has_ref = 0, is_ref = 0;
    DSV_FNUM fno = 0;
    PictureBody body;                // what the packet says behind the head (dec_parse.h); sym_first: within the decoder's list
    size_t stage_off = 0;
    bool dev_parse = false;          // the plane sections' symbols are parsed on the device (dec_parse_dev.hip) from body.head
    int cap[3] = {0, 0, 0};          // ... into lists of this many entries (min(header count, coefficients of the plane))
    size_t pkt_off = 0;              // ... out of the packet as staged at this offset of the round's stage block
    DSV_FRAME *of = nullptr; // output picture: a bordered frame on pinned memory the device writes directly (made in phase A), or none
    OutTarget target;        // ... where the picture goes: that frame, or (dsv2hip_dec_batch_device / _surface) the caller's device planes
    int out_format = 0;      // format of the delivered picture: the stream's, or 4:2:0 under out420p
    bool sharp = false;      // the decoder's postsharp switch when the packet was handed in
    int draw = 0;            // the decoder's draw_info when the packet was handed in: non-zero = overlay on the luma of `of` (overlay.hip)
};

struct DecScratch { // held by ONE device round at a time (pool below); owns the stream the round's kernels run on
    TableArena tabs;
    hipStream_t main = nullptr;
    hipStream_t main_stream()
    {
        if (!main) {
            HIPCHK(hipStreamCreateWithFlags(&main, hipStreamNonBlocking));
        }
        return main;
    }
    uint8_t *h_stage = nullptr, *d_stage = nullptr;
    size_t stage_cap = 0;
    void ensure_stage(size_t bytes)
    {
        if (bytes <= stage_cap) {
            return;
        }
        if (stage_cap) {
            HIPCHK(hipHostFree(h_stage));
            HIPCHK(hipFree(d_stage));
        }
        bytes += bytes / 4;
        HIPCHK(hipHostMalloc((void **) &h_stage, bytes, hipHostMallocDefault));
        HIPCHK(hipMalloc((void **) &d_stage, bytes));
        stage_cap = bytes;
    }
};
// process-wide pool, last released first (same reasoning as the encoder's ScratchPool): a lockstep group keeps getting the
// same scratch and stream from whatever thread it calls, and nothing is leaked when caller threads come and go
struct DecScratchPool {
    std::mutex mu;
    std::vector<DecScratch *> idle;
    bool primed = false;
    DecScratch *acquire(DecScratch *prefer) // (prefer: the one this thread used last, so that a group keeps its stream)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!primed) { // the first four scratches' streams are made once, in a row, and kept (see the encoder's ScratchPool)
            primed = true;
            DecScratch *first[4];
            for (int k = 0; k < 4; k++) {
                first[k] = new DecScratch();
                first[k]->main_stream();
            }
            for (int k = 3; k >= 0; k--) {
                idle.push_back(first[k]);
            }
        }
        if (idle.empty()) {
            return new DecScratch();
        }
        for (size_t i = 0; i < idle.size(); i++) {
            if (idle[i] == prefer) {
                idle.erase(idle.begin() + (ptrdiff_t) i);
                return prefer;
            }
        }
        DecScratch *sc = idle.back();
        idle.pop_back();
        return sc;
    }
    void release(DecScratch *sc)
    {
        std::lock_guard<std::mutex> lk(mu);
        idle.push_back(sc);
    }
};
DecScratchPool g_dec_scratch_pool;
thread_local DecScratch *t_last_dec_scratch = nullptr;
struct DecScratchLease {
    DecScratch *sc = g_dec_scratch_pool.acquire(t_last_dec_scratch);
    DecScratchLease() { t_last_dec_scratch = sc; }
    ~DecScratchLease() { g_dec_scratch_pool.release(sc); }
};

struct DecClock { // DSV2_TRACE=2: wall-clock split of a lockstep decode step, printed every 16 steps
    bool on = (trace_mode() & 2) != 0;
    double acc[6] = {0};
    int steps = 0;
    std::chrono::steady_clock::time_point t0;
    void start() { if (on) t0 = std::chrono::steady_clock::now(); }
    void lap(int i)
    {
        if (!on) return;
        auto t1 = std::chrono::steady_clock::now();
        acc[i] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
    void done(int n)
    {
        if (!on || ++steps % 16) return;
        fprintf(stderr, "[dec batch n=%d] ms/step: parse %.2f | pack %.2f | enqueue %.2f | wait %.2f | deliver %.2f\n", n, acc[0] / 16, acc[1] / 16,
                acc[2] / 16, acc[3] / 16, acc[4] / 16);
        for (double &a : acc) a = 0;
    }
};
thread_local DecClock t_dec_clock;
std::atomic<unsigned long long> g_uv_rounds[2]; // device rounds whose chroma interleave ran in the wide / the general form (dsv2hip_dec_surface_stats)
// ... whose RGB conversion of a layout (kRgbOut*) ran in the wide / the general form: dsv2hip_dec_rgb_stats (packed), _tensor_stats (planar),
// _hwc_stats (interleaved)
std::atomic<unsigned long long> g_rgb_rounds[kRgbOutLayouts][2];
std::atomic<unsigned long long> g_scale_rounds[2]; // ... whose reduction ran in the wide / the general form (dsv2hip_dec_scale_stats)
std::atomic<unsigned long long> g_resize_rounds[2]; // ... whose resampling ran in the wide / the general form (dsv2hip_dec_resize_stats)

// Where a picture's plane sections are parsed: DSV2_DEC_DEVICE_PARSE = 0: on the host (one pool task per picture: ~2 ms of a
// core per 1080p P picture -- the fastest decoder while there are ~16 host cores per GPU to burn); 1: P pictures on the device, one
// wavefront per section (dec_parse_dev.hip) -- slower per step, the section being one dependency chain, but with ~1.4 host cores
// per GPU instead of ~15 -- and intra pictures (1 in a GOP, ten times the symbols: a 0.4 s chain on a wavefront) on the host; 2:
// everything on the device (tests).  Unset: by the host budget of this process -- the device parses when fewer than 12 cores are
// usable (DSV2_DEC_PARSE_AUTO_CORES), e.g. eight ranks of an 8-GPU node on a 64-core host, or a rank pinned to two cores.
static int dev_parse_mode()
{
    if (const char *e = getenv("DSV2_DEC_DEVICE_PARSE")) {
        return atoi(e);
    }
    cpu_set_t set;
    CPU_ZERO(&set);
    const int need = getenv("DSV2_DEC_PARSE_AUTO_CORES") ? atoi(getenv("DSV2_DEC_PARSE_AUTO_CORES")) : 12;
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) < need) {
        return 1;
    }
    return 0;
}
static std::atomic<int> g_dev_parse{dev_parse_mode()};

// phase A: everything dsv_dec does before it touches the device (dsv_decoder.c:393-503).  The bit parsing itself is
// dec_parse.h (device-free: fuzzed on the CPU under AddressSanitizer by tests/parser_fuzz.cpp); here: the private copy of
// the packet, the device instance of the stream's geometry, the pinned mirrors the device reads.
void dec_parse(DecJob &jb)
{
    DSV_DECODER *d = jb.d;
    DSV_BUF *buffer = jb.buf;
    *jb.fn = (DSV_FNUM) -1;
    jb.draw = d->draw_info;
    // parse from a private copy with zeroed slack behind it, so that codes can be read through a 64-bit window
    static thread_local std::vector<uint8_t> copy;
    if (buffer->len > (1u << 28)) { // (bit positions are 32-bit)
        jb.ret = DSV_DEC_ERROR;
        return;
    }
    copy.assign(buffer->data, buffer->data + buffer->len);
    copy.resize((size_t) buffer->len + 64, 0);
    const uint8_t *pkt = copy.data();
    BitReader br{pkt, 0};
    br.wide = true;
    br.limit = (buffer->len + 8) * 8; // reads stop here; the copy is zero for 56 more bytes (see BitReader)
    PictureHead hd;
    const int rc = parse_head(br, d, hd);
    if (rc != kParsePicture) {
        jb.ret = rc;
        return;
    }
    const DSV_META *meta = &d->vidmeta;
    jb.has_ref = hd.has_ref;
    jb.is_ref = hd.is_ref;
    jb.fno = hd.fno;
    bind_device();
    DecImpl *im = (DecImpl *) d->ref;
    if (!im) {
        im = new DecImpl();
        d->ref = im;
    }
    jb.im = im;
    if (im->ready && (im->dev.w != meta->width || im->dev.h != meta->height || im->dev.format != meta->subsamp ||
                      im->dev.blk_w != hd.blk_w || im->dev.blk_h != hd.blk_h)) {
        im->destroy_dev(); // stream parameters changed: start over
        im->ready = false;
        im->have_ref = false;
    }
    if (!im->ready) {
        im->dev.init(meta->subsamp, meta->width, meta->height, hd.blk_w, hd.blk_h, 0, false);
        im->dev.scratch_uv[0].ensure((size_t) im->dev.cw[1] * im->dev.ch[1], sbt_ll_elems(im->dev.cw[1], im->dev.ch[1]));
        im->dev.scratch_uv[1].ensure((size_t) im->dev.cw[2] * im->dev.ch[2], sbt_ll_elems(im->dev.cw[2], im->dev.ch[2]));
        im->ready = true;
    }
    CodecDev &dv = im->dev;
    PictureBody &body = jb.body;
    const int dev_mode = g_dev_parse.load(std::memory_order_relaxed);
    jb.dev_parse = dev_mode >= 2 || (dev_mode == 1 && hd.has_ref);
    parse_body(br, pkt, hd.has_ref, dv.nbh, dv.nbv, dv.scan, im->side, im->pos, im->val, body, jb.dev_parse);
    if (jb.dev_parse) {
        // the symbol lists live in device memory; their sizes come from the (untrusted) header counts, bounded by the planes' coefficient counts
        size_t at = 0;
        for (int c = 0; c < 3; c++) {
            body.sym_first[c] = at;
            jb.cap[c] = body.ok[c] > 0 ? std::min(std::max(body.head[c].runs, 0), dv.scan[c].base[10]) : 0;
            at += (size_t) jb.cap[c];
        }
        dv.ensure_dev_syms(at);
    } else {
        // the device reads the symbols straight from pinned host memory (each is read exactly once)
        dv.ensure_host_syms(body.nsym);
        memcpy(dv.h_pos, im->pos.data(), body.nsym * sizeof(uint32_t));
        memcpy(dv.h_val, im->val.data(), body.nsym * sizeof(int32_t));
    }
    *jb.fn = jb.fno;
    if (jb.has_ref && !im->have_ref) {
        jb.ret = DSV_DEC_ERROR; /* reference frame not found (dsv_decoder.c:535) */
        return;
    }
    jb.out_format = im->out420p ? DSV_SUBSAMP_420 : meta->subsamp;
    jb.sharp = im->postsharp;
    if (jb.out) {
        jb.of = mk_frame_pinned(jb.out_format, meta->width, meta->height);
        jb.target = target_frame(jb.of);
    }
    jb.pic = true;
}

// ---- one device round: phases B and C for the pictures of one geometry, as functions over one Round ----
struct Slice { // a run of the sorted order with one (frame type, lossless) class: one set of dequantiser / transform launches
    int first, count, isP, lossless, max_seg[3][4];
};

// The way out of a round's pictures: the jobs of their plans (dec_delivery.h), one table per launch class -- a class that no picture of
// the round uses has no table and no launch -- and what picks each launch's form.
struct Delivery {
    Tab<CopyJob> copy;
    Tab<To420Job> to420;
    Tab<EgressJob> eg;
    Tab<OverlayJob> ov;
    Tab<ScaleOutJob> scl;
    Tab<ResizeOutJob> rsz;
    Tab<UvEgressJob> uv;
    Tab<RgbOutJob> rgb[kRgbOutLayouts]; // one table per layout, one launch each
    size_t room[7 + kRgbOutLayouts] = {}; // entries the round's plans need of each table, in the order above
    int n_copy = 0, n_to420 = 0, n_eg = 0, n_ov = 0, n_scl = 0, n_rsz = 0, n_uv = 0, n_rgb[kRgbOutLayouts] = {};
    bool eg_wide = true, eg_sharp = false, scl_wide = true, rsz_wide = true, uv_wide = true, uv_conv = false; // DeliveryPlan's, over the round
    bool rgb_wide[kRgbOutLayouts] = {true, true, true};
    int scl_rows = 0, rsz_rows = 0, rsz_cols = 0, uv_rows = 0;
    bool ov_vectors = false;         // some overlay job draws motion vectors
    std::vector<DPlane> sharp_drawn; // luma planes that are drawn on AND sharpened: sharpened in place behind the overlay
    size_t count(const std::vector<DeliveryPlan> &plans) // the arena bytes the tables of these plans take
    {
        for (const DeliveryPlan &p : plans) {
            const int n[7] = {p.n_copy, p.n_to420, p.n_eg, p.n_overlay, p.n_scl, p.n_rsz, p.n_uv};
            for (int k = 0; k < 7; k++) {
                room[k] += (size_t) n[k];
            }
            if (p.n_rgb) {
                room[7 + p.rgb[0].layout] += (size_t) p.n_rgb;
            }
        }
        return room[0] * sizeof(CopyJob) + room[1] * sizeof(To420Job) + room[2] * sizeof(EgressJob) + room[3] * sizeof(OverlayJob) +
               room[4] * sizeof(ScaleOutJob) + room[5] * sizeof(ResizeOutJob) + room[6] * sizeof(UvEgressJob) +
               (room[7] + room[8] + room[9]) * sizeof(RgbOutJob) + 10 * 16; // (16: each table's alignment)
    }
    void take(TableArena &tabs)
    {
        copy = Tab<CopyJob>(tabs, room[0]);
        to420 = Tab<To420Job>(tabs, room[1]);
        eg = Tab<EgressJob>(tabs, room[2]);
        ov = Tab<OverlayJob>(tabs, room[3]);
        scl = Tab<ScaleOutJob>(tabs, room[4]);
        rsz = Tab<ResizeOutJob>(tabs, room[5]);
        uv = Tab<UvEgressJob>(tabs, room[6]);
        for (int l = 0; l < kRgbOutLayouts; l++) {
            rgb[l] = Tab<RgbOutJob>(tabs, room[7 + l]);
        }
    }
    template <class T> static void append(Tab<T> &t, int &n, const T *jobs, int count)
    {
        std::copy_n(jobs, count, t.h + n);
        n += count;
    }
    // oj: the picture's overlay job but for its plane
    void add(const DeliveryPlan &p, OverlayJob oj)
    {
        append(copy, n_copy, p.copy, p.n_copy);
        append(to420, n_to420, p.to420, p.n_to420);
        append(eg, n_eg, p.eg, p.n_eg);
        append(scl, n_scl, p.scl, p.n_scl);
        append(rsz, n_rsz, p.rsz, p.n_rsz);
        append(uv, n_uv, p.uv, p.n_uv);
        if (p.n_rgb) {
            const int l = p.rgb[0].layout;
            append(rgb[l], n_rgb[l], p.rgb, p.n_rgb);
            rgb_wide[l] = rgb_wide[l] && p.rgb_wide;
        }
        eg_wide = eg_wide && p.eg_wide, eg_sharp = eg_sharp || p.eg_sharp;
        scl_wide = scl_wide && p.scl_wide, scl_rows = std::max(scl_rows, p.scl_rows);
        rsz_wide = rsz_wide && p.rsz_wide, rsz_rows = std::max(rsz_rows, p.rsz_rows), rsz_cols = std::max(rsz_cols, p.rsz_cols);
        uv_wide = uv_wide && p.uv_wide, uv_conv = uv_conv || p.uv_conv, uv_rows = std::max(uv_rows, p.uv_rows);
        if (p.n_overlay) {
            oj.dst = p.overlay[0];
            ov.h[n_ov++] = oj;
            ov_vectors = ov_vectors || (oj.isP && (oj.mode & DSV_DRAW_MOVECS));
            if (p.sharpen_overlaid) {
                sharp_drawn.push_back(oj.dst);
            }
        }
    }
    // h: the pictures' height; bytes: their reconstructions'
    void enqueue(hipStream_t bs, int w, int h, int nbh, int nbv, size_t bytes) const
    {
        copy_linear_batch(bs, copy.d, n_copy, bytes);
        to420_batch(bs, to420.d, n_to420, w, h);
        egress_batch(bs, eg.d, n_eg, h, eg_wide, eg_sharp);
        overlay_batch(bs, ov.d, n_ov, h, nbh, nbv, ov_vectors);
        for (const DPlane &pl : sharp_drawn) { // (a debugging combination: one launch a picture)
            post_process_plane(bs, pl);
        }
        if (n_scl) { // behind the overlay and the sharpening of the luma planes staged for it, in front of the two kernels that read what it stages
            egress_scale_batch(bs, scl.d, n_scl, scl_rows, scl_wide);
            g_scale_rounds[scl_wide ? 0 : 1]++;
        }
        if (n_rsz) { // (the same place in the order: a round may hold reduced and sized pictures side by side)
            egress_resize_batch(bs, rsz.d, n_rsz, rsz_cols, rsz_rows, rsz_wide);
            g_resize_rounds[rsz_wide ? 0 : 1]++;
        }
        if (n_uv) { // (chroma only: the overlay and the sharpening are none of its business, the reduction of a scaled picture's chroma is)
            egress_uv_batch(bs, uv.d, n_uv, uv_rows, uv_wide, uv_conv);
            g_uv_rounds[uv_wide ? 0 : 1]++;
        }
        for (int l = 0; l < kRgbOutLayouts; l++) { // last, packed, planar, interleaved: behind the overlay and the sharpening of the luma planes staged for it
            if (n_rgb[l]) {
                egress_rgb_batch(bs, rgb[l].d, n_rgb[l], h, l, rgb_wide[l]);
                g_rgb_rounds[l][rgb_wide[l] ? 0 : 1]++;
            }
        }
    }
};

struct Round { // what outlives a phase (the decoder's counterpart of the encoder's Step)
    DecJob *const jobs;
    const std::vector<int> &ids;
    const int n;
    DecScratchLease lease; // (the round ends with its stream drained: nothing of the scratch is in use after it)
    DecScratch &sc = *lease.sc;
    CodecDev &dv0; // the geometry every picture of the round shares
    hipStream_t bs = sc.main_stream(); // (a stream of the scratch pool, made once: see the encoder's ScratchPool)
    const size_t nb = dv0.nblocks(), mv_bytes = nb * sizeof(DSV_MV), bd_bytes = (nb + 15) & ~(size_t) 15;
    size_t stage_used = 0;
    std::vector<int> order; // ids, sorted by (frame type, lossless): the kernels are specialised on those.  order[slot] = job
    std::vector<Slice> slices;
    // coefficients.  Device-parsed sections: one parse job each; a damaged one raises its flag and the plane's residual is zeroed
    // behind the inverse transform (zcond); zfail: the residual planes of sections that the host found damaged
    Tab<CopyJob> zero, zcond, zfail;
    Tab<DequantJob> dq[3];
    Tab<PlaneJob> pj[3];
    Tab<DecParseJob> parse;
    Tab<int> fail;
    int n_parse = 0, n_zfail = 0;
    size_t max_coef_bytes = 0, max_plane_bytes = 0;
    // reconstruction
    Tab<McJob> mc_pred, mc_filt, mc_intra;
    Tab<PlanePair> icopy[3];
    Tab<DPlane> ext[3];
    int nP = 0, nI = 0, nIf = 0, n_ext = 0;
    bool any_filter = false;
    std::vector<DeliveryPlan> plans; // plans[slot]: the way out of the picture in that slot of `order` (dec_delivery.h)
    Delivery out;
    Round(DecJob *jobs_, const std::vector<int> &ids_) : jobs(jobs_), ids(ids_), n((int) ids_.size()), dv0(jobs_[ids_[0]].im->dev), order(ids_) {}
    const DSV_MV *d_mvs(const DecJob &jb) const { return (const DSV_MV *) (sc.d_stage + jb.stage_off); } // as staged for the kernels
    const uint8_t *d_bd(const DecJob &jb) const { return sc.d_stage + jb.stage_off + mv_bytes; }
};

// The arena holds every table of the round: the fixed tables, of which a picture has the entries below (8192 bytes reserved for them;
// the 65536 cover the tables' alignment), and on top the delivery tables, sized by the round's plans.  (Taking beyond what was reserved
// is fatal: TableArena::take.)
constexpr size_t kFixedEntryBytes = 3 * (3 * sizeof(CopyJob) /* zero, zfail, zcond */ + sizeof(DequantJob) + sizeof(PlaneJob) + sizeof(PlanePair) +
                                         sizeof(DPlane) + sizeof(McJob) /* mc_pred, mc_filt, mc_intra: one each */ + sizeof(DecParseJob) + sizeof(int));
static_assert(kFixedEntryBytes <= 8192, "a picture's entries in the round's fixed job tables outgrew the 8192 bytes reserved for them");
void round_take_tables(Round &r)
{
    TableArena &tabs = r.sc.tabs;
    const size_t n = (size_t) r.n;
    tabs.reserve(n * 8192 + 65536 + r.out.count(r.plans));
    r.zero = Tab<CopyJob>(tabs, 3 * n);
    for (int c = 0; c < 3; c++) {
        r.dq[c] = Tab<DequantJob>(tabs, n);
        r.pj[c] = Tab<PlaneJob>(tabs, n);
        r.icopy[c] = Tab<PlanePair>(tabs, n);
        r.ext[c] = Tab<DPlane>(tabs, n);
    }
    r.mc_pred = Tab<McJob>(tabs, n);
    r.mc_filt = Tab<McJob>(tabs, n);
    r.mc_intra = Tab<McJob>(tabs, n);
    r.zfail = Tab<CopyJob>(tabs, 3 * n);
    r.parse = Tab<DecParseJob>(tabs, 3 * n);
    r.zcond = Tab<CopyJob>(tabs, 3 * n);
    r.fail = Tab<int>(tabs, 3 * n);
    r.out.take(tabs);
}

size_t staged_len(const DSV_BUF *b) { return ((size_t) b->len + 64 + 15) & ~(size_t) 15; } // a packet as staged: 16-byte aligned, 64 zero bytes behind it

// stage layout: per stream {motion field, block flags}, then -- for pictures whose sections the device parses -- the packets
// (the parser reads a 2 KB window: the block ends with that much slack)
void round_stage(Round &r)
{
    size_t total = 0;
    int n_dev = 0;
    for (int k : r.ids) {
        r.jobs[k].stage_off = total;
        total += r.mv_bytes + r.bd_bytes;
    }
    for (int k : r.ids) {
        DecJob &jb = r.jobs[k];
        if (jb.dev_parse) {
            jb.pkt_off = total;
            total += staged_len(jb.buf);
            n_dev++;
        }
    }
    r.stage_used = total;
    r.sc.ensure_stage(total + (n_dev ? 4096 : 0));
    parallel_for(r.n, [&](int i) {
        DecJob &jb = r.jobs[r.ids[(size_t) i]];
        uint8_t *h = r.sc.h_stage + jb.stage_off;
        if (jb.has_ref) {
            memcpy(h, jb.im->mvs.data(), r.mv_bytes);
        }
        memcpy(h + r.mv_bytes, jb.im->blockdata.data(), r.nb);
        if (jb.dev_parse) {
            uint8_t *p = r.sc.h_stage + jb.pkt_off;
            memcpy(p, jb.buf->data, jb.buf->len);
            memset(p + jb.buf->len, 0, staged_len(jb.buf) - jb.buf->len);
        }
    });
    t_dec_clock.lap(1);
}

void round_sort(Round &r)
{
    auto cls = [&](int k) { return r.jobs[k].has_ref * 2 + r.jobs[k].body.lossless; };
    std::stable_sort(r.order.begin(), r.order.end(), [&](int a, int b) { return cls(a) > cls(b); });
    for (int i = 0; i < r.n; i++) {
        const DecJob &jb = r.jobs[r.order[(size_t) i]];
        if (r.slices.empty() || r.slices.back().isP != jb.has_ref || r.slices.back().lossless != jb.body.lossless) {
            r.slices.push_back(Slice{i, 0, jb.has_ref, jb.body.lossless, {}});
        }
        r.slices.back().count++;
    }
}

// zero, dequantise and inverse-transform jobs of the picture in slot i of slice sl; its device-parse jobs, its damaged planes
void fill_coef_jobs(Round &r, Slice &sl, int i, DecJob &jb)
{
    CodecDev &dv = jb.im->dev;
    const PictureBody &b = jb.body;
    DFrame &resid = dv.pred; // the decoder's residual picture
    for (int c = 0; c < 3; c++) {
        size_t cbytes = (size_t) dv.cw[c] * dv.ch[c] * sizeof(int32_t);
        r.zero.h[3 * i + c] = CopyJob{nullptr, dv.coefs[c], cbytes};
        r.max_coef_bytes = std::max(r.max_coef_bytes, cbytes);
        const CopyJob zero_resid = CopyJob{nullptr, resid.alloc + resid.plane_off[c], resid.plane_len[c]};
        DequantJob &dq = r.dq[c].h[i];
        dq.coefs = dv.coefs[c];
        // host-parsed symbols: read in place from pinned host memory; device-parsed: the kernel writes the counts into this record's device copy
        dq.pos = (jb.dev_parse ? dv.d_sym_pos : dv.h_pos) + b.sym_first[c];
        dq.val = (jb.dev_parse ? dv.d_sym_val : dv.h_val) + b.sym_first[c];
        for (int k = 0; k < 4; k++) {
            dq.seg[k] = jb.dev_parse ? 0 : b.seg[c][k];
            sl.max_seg[c][k] = std::max(sl.max_seg[c][k], jb.dev_parse ? jb.cap[c] : b.seg[c][k]);
        }
        if (jb.dev_parse && b.ok[c] > 0) {
            DecParseJob &pj = r.parse.h[r.n_parse];
            pj.pkt = r.sc.d_stage + jb.pkt_off;
            pj.data_bitpos = b.head[c].data_bitpos;
            pj.limit_bits = (jb.buf->len + 8) * 8;
            pj.end_byte = b.head[c].end_byte;
            pj.runs = b.head[c].runs;
            pj.cap = jb.cap[c];
            pj.chroma = c != 0;
            pj.pos = dv.d_sym_pos + b.sym_first[c];
            pj.val = dv.d_sym_val + b.sym_first[c];
            pj.seg_out = const_cast<int *>(r.dq[c].d[i].seg);
            pj.fail = const_cast<int *>(r.fail.d) + r.n_parse;
            r.fail.h[r.n_parse] = 0;
            r.zcond.h[r.n_parse] = zero_resid;
            r.max_plane_bytes = std::max(r.max_plane_bytes, resid.plane_len[c]);
            r.n_parse++;
        }
        dq.bd = r.d_bd(jb);
        dq.LL = b.LL[c];
        dequant_steps(&dq, dv.quant_cfg(c, jb.has_ref, b.lossless, 0, nullptr), b.quant);
        PlaneJob &pj = r.pj[c].h[i];
        pj = PlaneJob{};
        pj.pic = resid.p[c];
        pj.coefs = dv.coefs[c];
        for (int t = 0; t < 3; t++) {
            pj.t[t] = c ? dv.scratch_uv[c - 1].t[t] : dv.scratch.t[t];
        }
        pj.bd = r.d_bd(jb);
        pj.q = b.quant;
        if (b.ok[c] <= 0) { // "decoding error in plane": its residual plane stays zero (dsv_decoder.c:516-523)
            r.zfail.h[r.n_zfail++] = zero_resid;
            r.max_plane_bytes = std::max(r.max_plane_bytes, resid.plane_len[c]);
        }
    }
}

// prediction + in-loop filters or intra copy + intra filter, border extension of a picture that is kept as a reference
void fill_recon_jobs(Round &r, DecJob &jb)
{
    CodecDev &dv = jb.im->dev;
    PicSet &cur = dv.pics[jb.im->cur], &ref = dv.pics[jb.im->cur ^ 1];
    DFrame &resid = dv.pred;
    McJob mj;
    mj.mvs = r.d_mvs(jb);
    mj.bd = r.d_bd(jb);
    mj.p = dv.mc_params((int) (jb.fno % 2), jb.body.lossless);
    if (jb.has_ref) {
        mj.f = make_filter_params(mj.p, jb.body.quant, jb.body.do_filter, jb.d->vidmeta.inter_sharpen);
        for (int c = 0; c < 3; c++) {
            mj.ref.p[c] = ref.recon.p[c];
            mj.pred.p[c] = cur.recon.p[c];
            mj.res.p[c] = resid.p[c];
        }
        r.mc_pred.h[r.nP] = mj;
        mj.res = mj.pred;
        r.mc_filt.h[r.nP++] = mj;
        r.any_filter = r.any_filter || !jb.body.lossless;
    } else {
        mj.f = make_filter_params(mj.p, jb.body.quant, 1, 0);
        for (int c = 0; c < 3; c++) {
            mj.ref.p[c] = mj.pred.p[c] = mj.res.p[c] = resid.p[c];
            r.icopy[c].h[r.nI] = PlanePair{resid.p[c], cur.recon.p[c]};
        }
        r.nI++;
        if (jb.body.do_filter && !jb.body.lossless) { // dsv_intra_filter is a no-op for lossless pictures (bmc.c:398)
            r.mc_intra.h[r.nIf++] = mj;
        }
    }
    if (jb.is_ref || !jb.has_ref) {
        for (int c = 0; c < 3; c++) {
            r.ext[c].h[r.n_ext] = cur.recon.p[c];
        }
        r.n_ext++;
    }
}

// every picture's way out, planned (dec_delivery.h) before the tables are sized; the staging areas a plan needs are made here
void round_plan(Round &r)
{
    r.plans.reserve((size_t) r.n);
    for (int k : r.order) {
        const DecJob &jb = r.jobs[k];
        DecImpl &im = *jb.im;
        static const DPlane none = {nullptr, 0, 0, 0};
        const DPlane &luma = needs_staged_luma(jb.target, jb.sharp, jb.draw) ? im.staged_luma() : none;
        const DPlane *scaled = needs_staged_scaled(jb.target) ? im.staged_scaled(needs_staged_full(jb.target)) : nullptr;
        r.plans.push_back(plan_delivery(im.dev.pics[im.cur].recon, jb.out_format, jb.target, jb.sharp, jb.draw, luma, scaled));
    }
}

// (stage spans for bench.py's decode roofline: HIP events on this step's stream when dsv2hip_prof_enable(1) is on -- the
// encoder's stage names: QUANT = zero + scatter + dequantise, INV_SBT, RECON_FILTER = intra filter / motion-compensated
// reconstruction + in-loop filters, EXTEND = borders + the picture's way into the caller's frame)
thread_local StageProf t_dec_prof;

void round_enqueue(Round &r)
{
    StageProf &prof = t_dec_prof;
    const CodecDev &dv0 = r.dv0;
    const hipStream_t bs = r.bs;
    HIPCHK(hipMemcpyAsync(r.sc.d_stage, r.sc.h_stage, r.stage_used, hipMemcpyHostToDevice, bs));
    r.sc.tabs.upload(bs);
    prof.begin(bs, ST_QUANT);
    if (r.n_parse) {
        DecScanBases sb_l, sb_c;
        for (int k = 0; k < 11; k++) {
            sb_l.base[k] = dv0.scan[0].base[k];
            sb_c.base[k] = dv0.scan[1].base[k];
        }
        dec_parse_planes(bs, r.parse.d, r.n_parse, sb_l, sb_c);
    }
    zero_linear_batch(bs, r.zero.d, 3 * r.n, r.max_coef_bytes);
    for (const Slice &sl : r.slices) {
        for (int c = 0; c < 3; c++) {
            dequant_jobs(bs, r.dq[c].d + sl.first, sl.count, sl.max_seg[c], dv0.quant_cfg(c, sl.isP, sl.lossless, 0, nullptr));
        }
    }
    prof.end(bs, ST_QUANT, r.n);
    prof.begin(bs, ST_INV_SBT);
    for (const Slice &sl : r.slices) {
        for (int c = 0; c < 3; c++) {
            sbt_inverse_jobs(bs, r.pj[c].d + sl.first, sl.count, dv0.cw[c], dv0.ch[c], c, sl.isP, sl.lossless, dv0.nbh, dv0.nbv, true);
        }
    }
    prof.end(bs, ST_INV_SBT, r.n);
    prof.begin(bs, ST_RECON_FILTER);
    zero_linear_batch(bs, r.zfail.d, r.n_zfail, r.max_plane_bytes);
    zero_linear_if_batch(bs, r.zcond.d, r.fail.d, r.n_parse, r.max_plane_bytes);
    intra_filter_batch(bs, r.mc_intra.d, r.nIf, dv0.w, dv0.h);
    mc_add_pred_batch(bs, r.mc_pred.d, r.mc_filt.d, r.nP, dv0.nbh, dv0.nbv, r.any_filter, dv0.w, dv0.h, dv0.blk_w, dv0.blk_h,
                      DSV_FORMAT_H_SHIFT(dv0.format) == 1 && DSV_FORMAT_V_SHIFT(dv0.format) == 1);
    prof.end(bs, ST_RECON_FILTER, r.n);
    prof.begin(bs, ST_EXTEND);
    for (int c = 0; c < 3; c++) {
        const DPlane &pl = dv0.pics[0].recon.p[c];
        copy_planes_batch(bs, r.icopy[c].d, r.nI, pl.w, pl.h);
        extend_planes(bs, r.ext[c].d, r.n_ext, pl.w, pl.h);
    }
    r.out.enqueue(bs, dv0.w, dv0.h, dv0.nbh, dv0.nbv, dv0.pics[0].recon.bytes);
    prof.end(bs, ST_EXTEND, r.n);
    t_dec_clock.lap(2);
}

void round_finish(Round &r)
{
    stream_wait(r.bs);
    t_dec_prof.collect();
    t_dec_clock.lap(3);
    // phase C: the pictures are already in their output frames / the callers' device buffers
    for (int k : r.order) {
        DecJob &jb = r.jobs[k];
        if (jb.is_ref) {
            jb.im->cur ^= 1;
            jb.im->have_ref = true;
        }
        if (jb.of) {
            *jb.out = jb.of;
        }
        jb.ret = DSV_DEC_OK;
    }
}

void dec_device_round(DecJob *jobs, const std::vector<int> &ids)
{
    Round r(jobs, ids);
    round_sort(r);
    round_plan(r);
    round_take_tables(r);
    round_stage(r);
    for (Slice &sl : r.slices) {
        for (int i = sl.first; i < sl.first + sl.count; i++) {
            DecJob &jb = jobs[r.order[(size_t) i]];
            fill_coef_jobs(r, sl, i, jb);
            fill_recon_jobs(r, jb);
            const CodecDev &dv = jb.im->dev;
            r.out.add(r.plans[(size_t) i], OverlayJob{{}, r.d_mvs(jb), r.d_bd(jb), dv.nbh, dv.nbv, dv.blk_w, dv.blk_h, jb.draw, jb.has_ref});
        }
    }
    round_enqueue(r);
    round_finish(r);
}

void dec_batch(DecJob *jobs, int n)
{
    set_wait_fine(n <= 1); // (dev.cpp: a single stream is a latency chain, its waits poll finely)
    bind_device();
    t_dec_clock.start();
    parallel_for(n, [&](int k) { dec_parse(jobs[k]); });
    t_dec_clock.lap(0);
    std::vector<int> todo;
    for (int k = 0; k < n; k++) {
        if (jobs[k].pic) {
            todo.push_back(k);
        }
    }
    while (!todo.empty()) { // one round per picture geometry present in the step
        const CodecDev &g = jobs[todo[0]].im->dev;
        std::vector<int> ids, rest;
        for (int k : todo) {
            const CodecDev &dv = jobs[k].im->dev;
            bool same = dv.w == g.w && dv.h == g.h && dv.format == g.format && dv.blk_w == g.blk_w && dv.blk_h == g.blk_h;
            (same ? ids : rest).push_back(k);
        }
        dec_device_round(jobs, ids);
        todo.swap(rest);
    }
    t_dec_clock.lap(4);
    t_dec_clock.done(n);
    for (int k = 0; k < n; k++) {
        dsv_buf_free(jobs[k].buf); /* the decoder frees its input on every path (dsv_decoder.c:414,432,438,581) */
    }
}

Coalescer<DecJob> g_dec_queue; // dsv_dec callers share lockstep steps (batch.h)

// Plane sizes of the picture as this decoder delivers it (dsv_mk_frame's, frame.c:63-113, in the stream's format or 4:2:0 under
// out420p), as the rows of a surface of `layout`: false before the metadata or for a value that is no layout.  An RGB layout is one
// plane of 4 * w bytes a row, and no layout for a decoder that converts to 4:2:0: an RGB picture has no chroma planes to subsample.
// A layout with a DSV2HIP_SCALE_* value: the sizes of the reduced picture -- dsv_mk_frame's for ceil(w / n) x ceil(h / n), nested
// round-ups commuting -- and no layout either for a decoder that converts to 4:2:0.
bool surface_dims(DSV_DECODER *d, int layout, size_t row_bytes[3], int rows[3])
{
    const bool rgb = is_rgb_layout(layout);
    const int shift = layout_shift(layout), plain = layout_unscaled(layout);
    if (!d || !d->got_metadata || (plain != DSV2HIP_SURFACE_PLANAR && plain != DSV2HIP_SURFACE_SEMIPLANAR && !rgb)) {
        return false;
    }
    const DSV_META &m = d->vidmeta;
    const bool out420p = d->ref && ((DecImpl *) d->ref)->out420p;
    if (out420p && (rgb || shift)) {
        return false;
    }
    const int width = (m.width + (1 << shift) - 1) >> shift, height = (m.height + (1 << shift) - 1) >> shift;
    if (rgb) {
        row_bytes[0] = 4 * (size_t) width, rows[0] = height;
        row_bytes[1] = row_bytes[2] = 0, rows[1] = rows[2] = 0;
        return true;
    }
    const int fmt = out420p ? DSV_SUBSAMP_420 : m.subsamp;
    const int hs = DSV_FORMAT_H_SHIFT(fmt), vs = DSV_FORMAT_V_SHIFT(fmt);
    const size_t cw = (size_t) ((width + (1 << hs) - 1) >> hs);
    const int ch = (height + (1 << vs) - 1) >> vs;
    const bool semi = plain == DSV2HIP_SURFACE_SEMIPLANAR;
    row_bytes[0] = (size_t) width, rows[0] = height;
    row_bytes[1] = semi ? 2 * cw : cw, rows[1] = ch;
    row_bytes[2] = semi ? 0 : cw, rows[2] = semi ? 0 : ch;
    return true;
}

// ... of the picture delivered at out_w x out_h (dsv2hip_dec_batch_surface_sized): dsv_mk_frame's plane sizes for that picture in the
// stream's format.  False in addition for a layout with a scale value, a decoder that converts to 4:2:0, a size that is not positive or
// outside w / 8 .. w by h / 8 .. h, and a plane whose resampling the kernel's 32-bit sums do not hold (resize_allowed).
bool sized_dims(DSV_DECODER *d, int layout, int out_w, int out_h, size_t row_bytes[3], int rows[3])
{
    size_t full_rb[3];
    int full_rows[3];
    if (layout_shift(layout) || !surface_dims(d, layout, full_rb, full_rows)) {
        return false;
    }
    const DSV_META &m = d->vidmeta;
    if ((d->ref && ((DecImpl *) d->ref)->out420p) || !resize_allowed(m.width, m.height, out_w, out_h)) {
        return false;
    }
    const int hs = DSV_FORMAT_H_SHIFT(m.subsamp), vs = DSV_FORMAT_V_SHIFT(m.subsamp);
    const int cw = (m.width + (1 << hs) - 1) >> hs, ch = (m.height + (1 << vs) - 1) >> vs;
    const int ocw = (out_w + (1 << hs) - 1) >> hs, och = (out_h + (1 << vs) - 1) >> vs;
    if (!resize_allowed(cw, ch, ocw, och)) {
        return false;
    }
    if (is_rgb_layout(layout)) {
        row_bytes[0] = 4 * (size_t) out_w, rows[0] = out_h;
        row_bytes[1] = row_bytes[2] = 0, rows[1] = rows[2] = 0;
        return true;
    }
    const bool semi = layout == DSV2HIP_SURFACE_SEMIPLANAR;
    row_bytes[0] = (size_t) out_w, rows[0] = out_h;
    row_bytes[1] = semi ? 2 * (size_t) ocw : (size_t) ocw, rows[1] = och;
    row_bytes[2] = semi ? 0 : (size_t) ocw, rows[2] = semi ? 0 : och;
    return true;
}

// one lockstep step with every picture delivered into a frame of out[], or (no out) to the device planes the jobs name
int dec_batch_run(std::vector<DecJob> &jobs, DSV_DECODER **decs, DSV_BUF *bufs, DSV_FRAME **out, DSV_FNUM *fn, int *ret)
{
    int n = 0;
    for (DecJob &jb : jobs) {
        jb.d = decs[n];
        jb.buf = &bufs[n];
        jb.out = out ? &out[n] : nullptr;
        jb.fn = &fn[n];
        if (out) {
            out[n] = NULL;
        }
        n++;
    }
    dec_batch(jobs.data(), n);
    for (int k = 0; k < n; k++) {
        ret[k] = jobs[(size_t) k].ret;
    }
    return n;
}

void read_rounds(std::atomic<unsigned long long> (&rounds)[2], unsigned long long *out2, int reset) // the dsv2hip_dec_*_stats readers
{
    for (int i = 0; i < 2; i++) {
        if (out2) {
            out2[i] = rounds[i].load();
        }
        if (reset) {
            rounds[i].store(0);
        }
    }
}

int set_switch(DSV_DECODER *d, bool DecImpl::*sw, int on) // (a switch may be set before the first packet made the DecImpl)
{
    if (!d) {
        return -1;
    }
    if (!d->ref) {
        d->ref = new DecImpl();
    }
    ((DecImpl *) d->ref)->*sw = on != 0;
    return 0;
}

} // namespace

extern "C" {

void dsv_dec_free(DSV_DECODER *d)
{
    g_dec_queue.forget(d);
    if (d->ref) {
        DecImpl *im = (DecImpl *) d->ref;
        if (im->ready) {
            im->destroy_dev();
        }
        delete im;
        d->ref = NULL;
    }
}

DSV_META *dsv_get_metadata(DSV_DECODER *d)
{
    DSV_META *m = (DSV_META *) dsv_alloc(sizeof(DSV_META));
    memcpy(m, &d->vidmeta, sizeof(DSV_META));
    return m;
}

int dsv_dec(DSV_DECODER *d, DSV_BUF *buffer, DSV_FRAME **out, DSV_FNUM *fn) // dsv_decoder.c:393
{
    DecJob jb;
    jb.d = d;
    jb.buf = buffer;
    jb.out = out;
    jb.fn = fn;
    if (!Coalescer<DecJob>::enabled()) {
        dec_batch(&jb, 1);
        return jb.ret;
    }
    // concurrent callers (a decoder per thread) share one lockstep step; dec_batch itself sorts mixed geometries into rounds,
    // so every caller carries the same key
    g_dec_queue.submit(jb, 0, d, dec_batch);
    if (jb.ret == DSV_DEC_EOS || jb.ret == DSV_DEC_ERROR) { // (a caller that gives up after an error must not stay expected; one that goes on is seen again)
        g_dec_queue.forget(d);
    }
    return jb.ret;
}

/* what the submit queue of dsv_dec did so far (see dsv2hip_enc_queue_stats) */
void dsv2hip_dec_queue_stats(unsigned long long *out4, int reset)
{
    Coalescer<DecJob>::Stats st = g_dec_queue.stats();
    if (out4) {
        out4[0] = st.calls;
        out4[1] = st.steps;
        out4[2] = st.largest;
        out4[3] = st.waited_us;
    }
    if (reset) {
        g_dec_queue.reset_stats();
    }
}

/* every picture this decoder returns from now on is converted to 4:2:0 by the GPU while it is written to the output
 * frame -- what the reference CLI's -out420p does on the host afterwards (dsv_main.c:1030-1048, util.c:79-153) */
int dsv2hip_dec_set_out420p(DSV_DECODER *d, int on) { return set_switch(d, &DecImpl::out420p, on); }

int dsv2hip_dec_parse_mode(void) { return g_dev_parse.load(); }
int dsv2hip_dec_set_parse_mode(int mode)
{
    if (mode < 0) {
        mode = dev_parse_mode(); // back to the environment / the host budget
    }
    g_dev_parse.store(mode > 2 ? 2 : mode);
    return g_dev_parse.load();
}

// lockstep decode: packet bufs[k] on decoder decs[k]; ret[k], out[k], fn[k] are what dsv_dec would return
int dsv2hip_dec_batch(int n, DSV_DECODER **decs, DSV_BUF *bufs, DSV_FRAME **out, DSV_FNUM *fn, int *ret)
{
    if (n <= 0 || !decs || !bufs || !out || !fn || !ret) {
        return 0;
    }
    std::vector<DecJob> jobs((size_t) n);
    return dec_batch_run(jobs, decs, bufs, out, fn, ret);
}

/* -postsharp of the reference CLI (dsv_main.c:1058-1060, :1084-1089) inside the decoder: the luma of every picture handed out
 * from now on goes through dsv_post_process -- last, behind the 4:2:0 conversion and the draw_info overlay */
int dsv2hip_dec_set_postsharp(DSV_DECODER *d, int on) { return set_switch(d, &DecImpl::postsharp, on); }

size_t dsv2hip_dec_picture_bytes(DSV_DECODER *d)
{
    size_t rb[3]; // the packed picture is the planar surface without padding
    int rows[3];
    if (!surface_dims(d, DSV2HIP_SURFACE_PLANAR, rb, rows)) {
        return 0;
    }
    return rb[0] * (size_t) rows[0] + rb[1] * (size_t) rows[1] + rb[2] * (size_t) rows[2];
}

// dsv2hip_dec_batch with the pictures delivered, packed, to device memory: nothing is consumed unless every decoder that could
// yield a picture (it has metadata) brings a buffer that holds one
int dsv2hip_dec_batch_device(int n, DSV_DECODER **decs, DSV_BUF *bufs, void *const *dev_out, const size_t *dev_cap, DSV_FNUM *fn, int *ret)
{
    if (n <= 0 || !decs || !bufs || !dev_out || !dev_cap || !fn || !ret) {
        return -1;
    }
    for (int k = 0; k < n; k++) {
        if (!decs[k] || (decs[k]->got_metadata && (!dev_out[k] || dev_cap[k] < dsv2hip_dec_picture_bytes(decs[k])))) {
            return -1;
        }
    }
    std::vector<DecJob> jobs((size_t) n);
    for (int k = 0; k < n; k++) {
        size_t rb[3];
        int rows[3];
        if (surface_dims(decs[k], DSV2HIP_SURFACE_PLANAR, rb, rows)) {
            jobs[(size_t) k].target = target_packed(dev_out[k], rb, rows);
        }
    }
    return dec_batch_run(jobs, decs, bufs, nullptr, fn, ret);
}

int dsv2hip_dec_device_frame(DSV_DECODER *d, DSV_BUF *buf, void *dev_out, size_t dev_cap, DSV_FNUM *fn)
{
    int ret = DSV_DEC_ERROR;
    if (dsv2hip_dec_batch_device(1, &d, buf, &dev_out, &dev_cap, fn, &ret) != 1) {
        return -1;
    }
    return ret;
}

int dsv2hip_dec_surface_dims(DSV_DECODER *d, int layout, size_t row_bytes[3], int rows[3])
{
    if (!row_bytes || !rows) {
        return -1;
    }
    return surface_dims(d, layout, row_bytes, rows) ? 0 : -1;
}

// dsv2hip_dec_batch_device with a surface per decoder: nothing is consumed unless every decoder that could yield a picture (it
// has metadata) brings a surface that holds one.  out_w / out_h: the sizes of dsv2hip_dec_batch_surface_sized (0 x 0: not sized), or
// none at all
static int dec_batch_surface(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_surface *surf, const int *out_w, const int *out_h,
                             DSV_FNUM *fn, int *ret)
{
    if (n <= 0 || !decs || !bufs || !surf || !fn || !ret) {
        return -1;
    }
    std::vector<DecJob> jobs((size_t) n);
    for (int k = 0; k < n; k++) {
        if (!decs[k]) {
            return -1;
        }
        if (!decs[k]->got_metadata) {
            continue;
        }
        const dsv2hip_out_surface &sf = surf[k];
        const int ow = out_w ? out_w[k] : 0, oh = out_h ? out_h[k] : 0;
        const bool sized = ow != 0 || oh != 0;
        size_t rb[3];
        int rows[3];
        if (!(sized ? sized_dims(decs[k], sf.layout, ow, oh, rb, rows) : surface_dims(decs[k], sf.layout, rb, rows))) {
            return -1;
        }
        OutTarget &t = jobs[(size_t) k].target;
        if (!target_surface(sf, rb, rows, &t)) {
            return -1;
        }
        if (sized && (ow != decs[k]->vidmeta.width || oh != decs[k]->vidmeta.height)) { // (at the picture's own size: the plain delivery)
            t.ow = ow, t.oh = oh;
        }
    }
    return dec_batch_run(jobs, decs, bufs, nullptr, fn, ret);
}

int dsv2hip_dec_batch_surface(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_surface *surf, DSV_FNUM *fn, int *ret)
{
    return dec_batch_surface(n, decs, bufs, surf, nullptr, nullptr, fn, ret);
}

int dsv2hip_dec_sized_dims(DSV_DECODER *d, int layout, int out_w, int out_h, size_t row_bytes[3], int rows[3])
{
    if (!row_bytes || !rows) {
        return -1;
    }
    if (out_w == 0 && out_h == 0) { // not sized
        return surface_dims(d, layout, row_bytes, rows) ? 0 : -1;
    }
    return sized_dims(d, layout, out_w, out_h, row_bytes, rows) ? 0 : -1;
}

int dsv2hip_dec_batch_surface_sized(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_surface *surf, const int *out_w, const int *out_h,
                                    DSV_FNUM *fn, int *ret)
{
    if (!out_w || !out_h) {
        return -1;
    }
    return dec_batch_surface(n, decs, bufs, surf, out_w, out_h, fn, ret);
}

int dsv2hip_dec_surface_frame_sized(DSV_DECODER *d, DSV_BUF *buf, const dsv2hip_out_surface *surf, int out_w, int out_h, DSV_FNUM *fn)
{
    int ret = DSV_DEC_ERROR;
    if (dsv2hip_dec_batch_surface_sized(1, &d, buf, surf, &out_w, &out_h, fn, &ret) != 1) {
        return -1;
    }
    return ret;
}

int dsv2hip_dec_surface_frame(DSV_DECODER *d, DSV_BUF *buf, const dsv2hip_out_surface *surf, DSV_FNUM *fn)
{
    int ret = DSV_DEC_ERROR;
    if (dsv2hip_dec_batch_surface(1, &d, buf, surf, fn, &ret) != 1) {
        return -1;
    }
    return ret;
}

// Element size, CSC bits and size of a tensor delivery as dsv2hip_dec_tensor_dims documents them: the rows of one plane (the three are
// alike), and the size to resample to (0 x 0: none -- not sized, or sized at the picture's own size).  False wherever an RGBA surface
// of that size is refused, for an unknown element type and for exactly one size zero.
static bool tensor_dims(DSV_DECODER *d, int dtype, int out_w, int out_h, size_t *row_bytes, int *rows, int *ow, int *oh)
{
    if (dtype != DSV2HIP_TENSOR_U8 && dtype != DSV2HIP_TENSOR_F16 && dtype != DSV2HIP_TENSOR_BF16 && dtype != DSV2HIP_TENSOR_F32) {
        return false;
    }
    size_t rb[3];
    int rw[3];
    const bool sized = out_w != 0 || out_h != 0;
    if (!(sized ? sized_dims(d, DSV2HIP_SURFACE_RGBA, out_w, out_h, rb, rw) : surface_dims(d, DSV2HIP_SURFACE_RGBA, rb, rw))) {
        return false;
    }
    *row_bytes = rb[0] / 4 * (size_t) tensor_elem(dtype), *rows = rw[0];
    const bool resample = sized && (out_w != d->vidmeta.width || out_h != d->vidmeta.height);
    *ow = resample ? out_w : 0, *oh = resample ? out_h : 0;
    return true;
}

int dsv2hip_dec_tensor_dims(DSV_DECODER *d, int dtype, int out_w, int out_h, size_t *row_bytes, int *rows)
{
    int ow, oh;
    if (!row_bytes || !rows) {
        return -1;
    }
    return tensor_dims(d, dtype, out_w, out_h, row_bytes, rows, &ow, &oh) ? 0 : -1;
}

// dsv2hip_dec_batch_surface's mirror for tensors: nothing is consumed unless every decoder that could yield a picture (it has metadata)
// brings a tensor that holds one
int dsv2hip_dec_batch_tensor(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_tensor *tens, DSV_FNUM *fn, int *ret)
{
    if (n <= 0 || !decs || !bufs || !tens || !fn || !ret) {
        return -1;
    }
    std::vector<DecJob> jobs((size_t) n);
    for (int k = 0; k < n; k++) {
        if (!decs[k]) {
            return -1;
        }
        if (!decs[k]->got_metadata) {
            continue;
        }
        const dsv2hip_out_tensor &tn = tens[k];
        size_t rb;
        int rows, ow, oh;
        if ((tn.csc & ~(DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE)) || !tensor_dims(decs[k], tn.dtype, tn.out_w, tn.out_h, &rb, &rows, &ow, &oh)) {
            return -1;
        }
        OutTarget &t = jobs[(size_t) k].target;
        if (!target_tensor(tn, rb, rows, &t)) {
            return -1;
        }
        t.ow = ow, t.oh = oh;
    }
    return dec_batch_run(jobs, decs, bufs, nullptr, fn, ret);
}

int dsv2hip_dec_tensor_frame(DSV_DECODER *d, DSV_BUF *buf, const dsv2hip_out_tensor *t, DSV_FNUM *fn)
{
    int ret = DSV_DEC_ERROR;
    if (dsv2hip_dec_batch_tensor(1, &d, buf, t, fn, &ret) != 1) {
        return -1;
    }
    return ret;
}

// Element size, CSC bits and size of an interleaved tensor delivery as dsv2hip_dec_hwc_dims documents them: tensor_dims' with three
// elements a pixel
static bool hwc_dims(DSV_DECODER *d, int dtype, int out_w, int out_h, size_t *row_bytes, int *rows, int *ow, int *oh)
{
    if (!tensor_dims(d, dtype, out_w, out_h, row_bytes, rows, ow, oh)) {
        return false;
    }
    *row_bytes *= 3;
    return true;
}

int dsv2hip_dec_hwc_dims(DSV_DECODER *d, int dtype, int out_w, int out_h, size_t *row_bytes, int *rows)
{
    int ow, oh;
    if (!row_bytes || !rows) {
        return -1;
    }
    return hwc_dims(d, dtype, out_w, out_h, row_bytes, rows, &ow, &oh) ? 0 : -1;
}

// dsv2hip_dec_batch_tensor's mirror for interleaved tensors
int dsv2hip_dec_batch_hwc(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_hwc *hws, DSV_FNUM *fn, int *ret)
{
    if (n <= 0 || !decs || !bufs || !hws || !fn || !ret) {
        return -1;
    }
    std::vector<DecJob> jobs((size_t) n);
    for (int k = 0; k < n; k++) {
        if (!decs[k]) {
            return -1;
        }
        if (!decs[k]->got_metadata) {
            continue;
        }
        const dsv2hip_out_hwc &hw = hws[k];
        size_t rb;
        int rows, ow, oh;
        if ((hw.csc & ~(DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE)) || !hwc_dims(decs[k], hw.dtype, hw.out_w, hw.out_h, &rb, &rows, &ow, &oh)) {
            return -1;
        }
        OutTarget &t = jobs[(size_t) k].target;
        if (!target_hwc(hw, rb, rows, &t)) {
            return -1;
        }
        t.ow = ow, t.oh = oh;
    }
    return dec_batch_run(jobs, decs, bufs, nullptr, fn, ret);
}

int dsv2hip_dec_hwc_frame(DSV_DECODER *d, DSV_BUF *buf, const dsv2hip_out_hwc *t, DSV_FNUM *fn)
{
    int ret = DSV_DEC_ERROR;
    if (dsv2hip_dec_batch_hwc(1, &d, buf, t, fn, &ret) != 1) {
        return -1;
    }
    return ret;
}

void dsv2hip_dec_hwc_stats(unsigned long long *out2, int reset) { read_rounds(g_rgb_rounds[kRgbOutInterleaved], out2, reset); }
void dsv2hip_dec_rgb_stats(unsigned long long *out2, int reset) { read_rounds(g_rgb_rounds[kRgbOutPacked], out2, reset); }
void dsv2hip_dec_tensor_stats(unsigned long long *out2, int reset) { read_rounds(g_rgb_rounds[kRgbOutPlanar], out2, reset); }
void dsv2hip_dec_scale_stats(unsigned long long *out2, int reset) { read_rounds(g_scale_rounds, out2, reset); }
void dsv2hip_dec_resize_stats(unsigned long long *out2, int reset) { read_rounds(g_resize_rounds, out2, reset); }
void dsv2hip_dec_surface_stats(unsigned long long *out2, int reset) { read_rounds(g_uv_rounds, out2, reset); }

} // extern "C"
