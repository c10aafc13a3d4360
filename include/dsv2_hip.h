/*
 * dsv2_hip.h -- C ABI of libdsv2hip.so, the MI355X (gfx950) implementation of the
 * DSV2 v2.8 per-frame encode/decode hot path.
 *
 * The library is a drop-in for the reference codec library: it exports the same
 * symbols with the same struct layouts, ownership rules and return codes, so the
 * reference's own CLI (src/dsv_main.c) links against it unchanged.
 * Each declaration cites the reference interface it replaces.
 *
 *   Section 1  shared types                  (reference src/dsv.h:100-273, dsv_internal.h:40-47)
 *   Section 2  encoder API                   (reference src/dsv_encoder.h:68-199)
 *   Section 3  decoder API                   (reference src/dsv_decoder.h:30-61)
 *   Section 4  frame / buffer / misc helpers (reference src/dsv.h:224-324)
 *   Section 5  hot-path seam on HOST buffers (reference src/dsv_internal.h:112-147, dsv.h:232-237)
 *              same signatures as the reference's internal functions; each call
 *              uploads its operands to HBM, runs the HIP kernels, downloads the result.
 *   Section 6  hot-path seam on DEVICE-resident buffers (dsv2hip_*), used by the
 *              encoder/decoder internally and by bench.py (inputs already in HBM).
 *
 * There is no CPU fallback: every compute entry point aborts with a message on
 * stderr when no HIP device is usable.
 */
#ifndef DSV2_HIP_H
#define DSV2_HIP_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Section 1: shared types                                                   */

/* packet types, dsv.h:38-45 */
#define DSV_PT_META 0x00
#define DSV_PT_PIC 0x04
#define DSV_PT_EOS 0x10
#define DSV_PACKET_HDR_SIZE 14
#define DSV_PACKET_TYPE_OFFSET 5
#define DSV_PACKET_PREV_OFFSET 6
#define DSV_PACKET_NEXT_OFFSET 10

/* chroma subsampling codes, dsv.h:78-96: bits 3..2 = horizontal shift, bits 1..0 = vertical shift */
#define DSV_SUBSAMP_444 0x0
#define DSV_SUBSAMP_422 0x4
#define DSV_SUBSAMP_420 0x5
#define DSV_SUBSAMP_411 0x8
#define DSV_SUBSAMP_410 0xA
#define DSV_SUBSAMP_UYVY 0x14
#define DSV_FORMAT_H_SHIFT(f) (((f) >> 2) & 0x3)
#define DSV_FORMAT_V_SHIFT(f) ((f) & 0x3)

#define DSV_MIN_BLOCK_SIZE 16
#define DSV_MAX_BLOCK_SIZE 32
#define DSV_MAX_QP_BITS 12
#define DSV_MAX_QP ((1 << DSV_MAX_QP_BITS) - 1)

typedef uint32_t DSV_FNUM;

typedef struct { /* dsv.h:100-119 */
    int width, height, subsamp;
    int fps_num, fps_den;
    int aspect_num, aspect_den;
    int inter_sharpen;
    int reserved;
} DSV_META;

typedef struct { /* dsv.h:121-127 */
    uint8_t *data; /* pixel (0,0); bordered planes have 32 valid pixels on every side */
    int len;
    int format;
    int stride;
    int w, h;
} DSV_PLANE;

typedef int32_t DSV_SBC; /* subband coefficient */
typedef struct {         /* dsv.h:131-135 */
    DSV_SBC *data;
    int width, height;
} DSV_COEFS;

typedef struct { /* dsv.h:137-149 */
    uint8_t *alloc;
    DSV_PLANE planes[3];
    int refcount;
    int format;
    int width, height;
    int border;
} DSV_FRAME;

/* motion vector / per-block mode record, 16 bytes, dsv.h:171-216 */
typedef struct {
    union {
        struct {
            int16_t x, y; /* quarter-pel units */
        } mv;
        int32_t all;
    } u;
    uint32_t flags; /* DSV_MV_BIT_* */
    uint16_t err;
    uint16_t dc; /* bit 8 (DSV_SRC_DC_PRED): low byte is a transmitted DC */
    uint8_t submask;
} DSV_MV;

#define DSV_MV_BIT_INTRA 0
#define DSV_MV_BIT_EPRM 1
#define DSV_MV_BIT_MAINTAIN 2
#define DSV_MV_BIT_SKIP 3
#define DSV_MV_BIT_RINGING 4
#define DSV_MV_BIT_NOXMITY 5
#define DSV_MV_BIT_NOXMITC 6
#define DSV_MV_BIT_SIMCMPLX 7
#define DSV_SRC_DC_PRED 0x100
#define DSV_MASK_ALL_INTRA 0xF

typedef struct { /* dsv.h:239-266 */
    DSV_META *vidmeta;
    int effort;
    int do_psy;
    int is_ref;
    int has_ref;
    int blk_w, blk_h;
    int nblocks_h, nblocks_v;
    int temporal_mc;
    int lossless;
    int reserved;
} DSV_PARAMS;

typedef struct { /* dsv.h:268-271 */
    uint8_t *data;
    unsigned len;
} DSV_BUF;

typedef struct { /* dsv_internal.h:40-47 */
    DSV_PARAMS *params;
    DSV_MV *mvs;
    uint8_t *blockdata; /* per-block DSV_IS_* flag bytes */
    uint8_t cur_plane;
    uint8_t isP;
    DSV_FNUM fnum;
} DSV_FMETA;

typedef struct { /* dsv_internal.h:49-52, MSB-first bit cursor */
    uint8_t *start;
    unsigned pos;
} DSV_BS;

/* per-block flag bits in DSV_FMETA.blockdata, dsv_internal.h:96-110 */
#define DSV_IS_STABLE 0x01
#define DSV_IS_MAINTAIN 0x02
#define DSV_IS_SKIP 0x04
#define DSV_IS_RINGING 0x08
#define DSV_IS_INTRA 0x10
#define DSV_IS_EPRM 0x20
#define DSV_IS_SIMCMPLX 0x40

/* ------------------------------------------------------------------------- */
/* Section 2: encoder (dsv_encoder.h)                                        */

#define DSV_ENCODER_VERSION 14
#define DSV_GOP_INTRA 0
#define DSV_GOP_INF 0x7fffffff
#define DSV_ENC_NUM_BUFS 0x03
#define DSV_ENC_FINISHED 0x04
#define DSV_MIN_EFFORT 0
#define DSV_MAX_EFFORT 10
#define DSV_RATE_CONTROL_CRF 0
#define DSV_RATE_CONTROL_ABR 1
#define DSV_RATE_CONTROL_CQP 2
#define DSV_MAX_PYRAMID_LEVELS 5
#define DSV_RC_QUAL_SCALE 4
#define DSV_MAX_QUALITY 100
#define DSV_RC_QUAL_MAX (DSV_MAX_QUALITY * DSV_RC_QUAL_SCALE)
#define DSV_USER_QUAL_TO_RC_QUAL(u) ((u) * DSV_RC_QUAL_SCALE)

#define DSV_PSY_ADAPTIVE_QUANT (1 << 0)
#define DSV_PSY_CONTENT_ANALYSIS (1 << 1)
#define DSV_PSY_I_VISUAL_MASKING (1 << 2)
#define DSV_PSY_P_VISUAL_MASKING (1 << 3)
#define DSV_PSY_ADAPTIVE_RINGING (1 << 4)
#define DSV_PSY_ALL 0xff

struct DSV_STATS { /* dsv_encoder.h:116-147 */
    unsigned inum, pnum, iqual, pqual, iminq, pminq, imaxq, pmaxq;
    unsigned isize, psize, imins, pmins, imaxs, pmaxs;
    unsigned mb, mbI, mbP, mbdc, mbsub;
    unsigned mbsubs[4];
    unsigned eprm, skip;
    unsigned fpx, hpx, qpx, fpy, hpy, qpy;
    unsigned ifnum, pfnum;
};

struct DSV_STAB_ACC {
    int32_t x, y;
};

/* Configuration is by writing the public fields between dsv_enc_init and dsv_enc_start,
 * exactly as with the reference (dsv_encoder.h:68-188).  The fields after `stats` are
 * internal state; `ref` holds this library's device-side encoder context. */
typedef struct {
    int quality;
    int effort;
    int gop;
    int do_scd;
    int do_temporal_aq;
    int do_psy;
    int do_dark_intra_boost;
    int do_intra_filter;
    int do_inter_filter;
    int skip_block_thresh;
    int block_size_override_x;
    int block_size_override_y;
    int variable_i_interval;
    int rc_mode;
    unsigned bitrate;
    int rc_pergop;
    int min_q_step;
    int max_q_step;
    int min_quality;
    int max_quality;
    int min_I_frame_quality;
    int prev_I_frame_quality;
    int intra_pct_thresh;
    int scene_change_pct;
    unsigned stable_refresh;
    int pyramid_levels;
    struct DSV_STATS stats;

    unsigned rc_qual;
    unsigned rf_total;
    unsigned rf_reset;
    int rf_avg;
    int total_P_frame_q;
    int avg_P_frame_q;
    int prev_complexity;
    int curr_complexity;
    int curr_avgmot;
    int curr_intra_pct;
    int curr_scblocks;
    int prev_chaos;
    int motion_chaos;
    int motion_static;
    int avg_err;
    int auto_filter;

    void (*frame_callback)(DSV_META *m, DSV_FRAME *orig, DSV_FRAME *recon);

    DSV_FNUM next_fnum;
    void *ref; /* reference: DSV_ENCDATA*; here: opaque device encoder context */
    DSV_META vidmeta;
    int prev_link;
    int force_metadata;
    struct DSV_STAB_ACC *stability;
    unsigned refresh_ctr;
    uint8_t *blockdata;
    uint8_t *intra_map;
    DSV_FNUM prev_gop;
    int prev_quant;
} DSV_ENCODER;

void dsv_enc_init(DSV_ENCODER *enc);                         /* dsv_encoder.h:190, dsv_encoder.c:1320 */
void dsv_enc_free(DSV_ENCODER *enc);                         /* dsv_encoder.h:191 */
void dsv_enc_set_metadata(DSV_ENCODER *enc, DSV_META *md);   /* dsv_encoder.h:192 */
void dsv_enc_force_metadata(DSV_ENCODER *enc);               /* dsv_encoder.h:193 */
void dsv_enc_start(DSV_ENCODER *enc);                        /* dsv_encoder.h:195 */
/* consumes `frame` (one reference), returns 1 or 2 packets in bufs[] (metadata first);
 * the caller frees each with dsv_buf_free: dsv_encoder.h:198, dsv_encoder.c:1431 */
int dsv_enc(DSV_ENCODER *enc, DSV_FRAME *frame, DSV_BUF *bufs);
void dsv_enc_end_of_stream(DSV_ENCODER *enc, DSV_BUF *bufs); /* dsv_encoder.h:199 */

/* ------------------------------------------------------------------------- */
/* Section 3: decoder (dsv_decoder.h)                                        */

#define DSV_DECODER_VERSION 2
#define DSV_DRAW_STABHQ 1
#define DSV_DRAW_MOVECS 2
#define DSV_DRAW_IBLOCK 4

typedef struct { /* dsv_decoder.h:39-45; zero-initialised by the caller */
    DSV_META vidmeta;
    void *ref; /* reference: DSV_IMAGE*; here: opaque device decoder context */
    /* DSV_DRAW_* bits, read by every dsv_dec call; honoured as in dsv_decoder.c:240-350, :555-561: any non-zero value draws
     * the block grid on the luma of the returned picture, the bits add dashes, vectors and intra marks; the picture later
     * P pictures predict from is never drawn on.  The reference stores the intra marks without a bounds check (:326-346);
     * here a mark that falls outside the luma plane (clipped last block row / column) is dropped. */
    int draw_info;
    int got_metadata;
} DSV_DECODER;

#define DSV_DEC_OK 0
#define DSV_DEC_ERROR 1
#define DSV_DEC_EOS 2
#define DSV_DEC_GOT_META 3
#define DSV_DEC_NEED_NEXT 4

/* frees `buf`; on DSV_DEC_OK with a picture packet *out holds one reference the caller
 * releases with dsv_frame_ref_dec: dsv_decoder.h:54, dsv_decoder.c:394 */
int dsv_dec(DSV_DECODER *d, DSV_BUF *buf, DSV_FRAME **out, DSV_FNUM *fn);
DSV_META *dsv_get_metadata(DSV_DECODER *d); /* dsv_alloc'd copy, dsv_decoder.h:58 */
void dsv_dec_free(DSV_DECODER *d);          /* dsv_decoder.h:61 */

/* ------------------------------------------------------------------------- */
/* Section 4: helpers (dsv.h:224-324)                                        */

void dsv_mk_coefs(DSV_COEFS *c, int format, int width, int height);
DSV_FRAME *dsv_mk_frame(int format, int width, int height, int border);
DSV_FRAME *dsv_load_planar_frame(int format, void *data, int width, int height);
DSV_FRAME *dsv_frame_ref_inc(DSV_FRAME *frame);
void dsv_frame_ref_dec(DSV_FRAME *frame);
DSV_FRAME *dsv_clone_frame(DSV_FRAME *f, int border);
void dsv_plane_xy(DSV_FRAME *f, DSV_PLANE *out, int c, int x, int y);
void dsv_mk_buf(DSV_BUF *buf, int size);
void dsv_buf_free(DSV_BUF *buf);
void *dsv_alloc(int size); /* zero-initialised */
void dsv_free(void *ptr);
void dsv_memory_report(void);
void dsv_set_log_level(int level);
int dsv_get_log_level(void);
int dsv_lb2(unsigned n);
int dsv_yuv_write(FILE *out, int fno, DSV_PLANE *p);
int dsv_yuv_write_seq(FILE *out, DSV_PLANE *p);
int dsv_yuv_read(FILE *in, int fno, uint8_t *o, int w, int h, int subsamp);
int dsv_yuv_read_seq(FILE *in, uint8_t *o, int w, int h, int subsamp);
void dsv_post_process(DSV_PLANE *dp); /* decoder-side sharpen, dsv_internal.h:147 */
extern char *dsv_lvlname[5];

/* ------------------------------------------------------------------------- */
/* Section 5: hot-path seam, HOST buffers in / out (kernels run on the GPU)  */

void dsv_fwd_sbt(DSV_PLANE *src, DSV_COEFS *dst, DSV_FMETA *fm);           /* sbt.c:848 */
void dsv_inv_sbt(DSV_PLANE *dst, DSV_COEFS *src, int q, DSV_FMETA *fm);    /* sbt.c:890 */
void dsv_encode_plane(DSV_BS *bs, DSV_COEFS *src, int q, DSV_FMETA *fm);   /* hzcc.c:586 */
int dsv_decode_plane(DSV_BS *bs, DSV_COEFS *dst, int q, DSV_FMETA *fm);    /* hzcc.c:617 */
void dsv_sub_pred(DSV_MV *mv, DSV_PARAMS *p, DSV_FRAME *pred, DSV_FRAME *resd, DSV_FRAME *ref); /* bmc.c:1058 */
void dsv_add_res(DSV_MV *mv, DSV_FMETA *fm, int q, DSV_FRAME *resd, DSV_FRAME *pred, int do_filter); /* bmc.c:1073 */
void dsv_add_pred(DSV_MV *mv, DSV_FMETA *fm, int q, DSV_FRAME *resd, DSV_FRAME *out, DSV_FRAME *ref,
                  int do_filter);                                          /* bmc.c:1094 */
void dsv_intra_filter(int q, DSV_PARAMS *p, DSV_FMETA *fm, int c, DSV_PLANE *dp, int do_filter); /* bmc.c:391 */
DSV_MV *dsv_intra_analysis(DSV_FRAME *src, DSV_PARAMS *params);            /* hme.c:1836 */
void dsv_frame_copy(DSV_FRAME *dst, DSV_FRAME *src);                       /* frame.c:186 */
void dsv_ds2x_frame_luma(DSV_FRAME *dst, DSV_FRAME *src);                  /* frame.c:211 */
DSV_FRAME *dsv_extend_frame(DSV_FRAME *frame);                             /* frame.c:423 */
DSV_FRAME *dsv_extend_frame_luma(DSV_FRAME *frame);                        /* frame.c:413 */

/* reference dsv_encoder.h:202-215; src/ref/ogr[0] are full-size frames, [1..levels] the pyramid */
typedef struct {
    DSV_PARAMS *params;
    DSV_FRAME *src[DSV_MAX_PYRAMID_LEVELS + 1];
    DSV_FRAME *ref[DSV_MAX_PYRAMID_LEVELS + 1];
    DSV_FRAME *ogr[DSV_MAX_PYRAMID_LEVELS + 1];
    DSV_MV *mvf[DSV_MAX_PYRAMID_LEVELS + 1];
    DSV_MV *ref_mvf;
    DSV_MV mv_bank[128];
    int n_mv_bank_used;
    DSV_ENCODER *enc;
    int quant;
} DSV_HME;
int dsv_hme(DSV_HME *hme, int *scene_change_blocks, int *avg_err);         /* hme.c:2001 */

/* ------------------------------------------------------------------------- */
/* Section 6: library-specific entry points                                  */

/* 0 when a gfx950 device is usable, else a negative code; never falls back to the CPU */
int dsv2hip_device_ok(void);
const char *dsv2hip_version(void);
/* select the HIP device used by contexts created afterwards on this thread (one process per GPU: LOCAL_RANK) */
int dsv2hip_set_device(int ordinal);

/* dsv_enc for a packed planar 8-bit picture (Y, U, V back to back, no padding) that already
 * lives in device memory: the picture is not copied from the host.  Used by bench.py so that
 * the timed region starts with inputs resident in HBM. */
int dsv2hip_enc_device_frame(DSV_ENCODER *enc, const void *dev_planar, DSV_BUF *bufs);
/* lockstep step over n independent encoders of identical geometry: one frame each, the latency-bound
 * kernels (motion-estimation fronts, MC, in-loop filters) are launched once for all streams.  bufs has
 * 4 slots per stream; nbufs[k] = packets of stream k.  Output is identical to n separate dsv_enc calls.
 * WHAT A STEP MUST SHARE (this call, _batch_surface and _batch_host alike; the submit queue behind dsv_enc groups callers by the
 * same rule): vidmeta.width, .height and .subsamp; block_size_override_x and _y; the pyramid depth the encoder runs with
 * (pyramid_levels, or what 0 resolves to for the picture: an encoder that says 3 and one that says 0 at a size that resolves to 3
 * agree); do_psy.  A step whose encoders differ in one of these is refused as a whole with -1 before any encoder, frame counter,
 * input buffer or nbufs entry is touched; the encoders stay usable, each in steps of its own kind.
 * EVERYTHING ELSE IS PER STREAM and may differ freely within one step: quality (lossless streams beside lossy ones), effort, gop and
 * the phase within it, the frame number (streams may join a step group late, leave early, or sit steps out), rc_mode, bitrate and
 * the quality bounds, skip_block_thresh, do_scd, do_temporal_aq, do_dark_intra_boost, do_intra_filter, do_inter_filter,
 * variable_i_interval, scene_change_pct, intra_pct_thresh, stable_refresh, and the metadata's fps and inter_sharpen.  An encoder
 * may also change its company, its slot and its entry point from one picture to the next -- dsv_enc, _enc_device_frame, _enc_batch,
 * _batch_host and _batch_surface in any order: its packets are those of dsv_enc on its pictures alone
 * (tests/test_gpu_enc_mixed_steps.py). */
int dsv2hip_enc_batch(int n, DSV_ENCODER **encs, const void *const *dev_planar, DSV_BUF *bufs, int *nbufs);
/* The same step for pictures that are SURFACES with a row pitch in device memory -- what hardware video decoders, capture
 * pipelines, image libraries and hipMallocPitch hand out -- read in place: no repacking pass, no trip through the host.
 *   PLANAR:     plane[0..2] = Y, U, V, row y of plane c at plane[c] + y * pitch[c].
 *   SEMIPLANAR: plane[0] = Y, plane[1] = one interleaved chroma plane, rows of 2 * cw bytes U0 V0 U1 V1 ...; plane[2] and pitch[2]
 *               are ignored.  Allowed for every chroma format: NV12 with 4:2:0, NV16 with 4:2:2, NV24 with 4:4:4.
 * Plane sizes are dsv_mk_frame's for the stream's format: luma w x h, chroma cw x ch (the format's shifts, rounded up).  Any pointer
 * alignment and any pitch >= the row's bytes (w, cw, or 2 * cw for the interleaved plane) is accepted; the surfaces of one step may
 * differ in layout, pitch and alignment (16-byte aligned pointers and pitches with row bytes a multiple of 16 throughout the step
 * take the fast form of the ingest).  A packed picture is the planar surface with pitch = {w, cw, cw}.  The surface is only read,
 * and only inside its rows: padding between rows may hold anything, the last row needs none behind it.  surf[k] itself is
 * copied: the array need not outlive the call.
 * dsv2hip_enc_batch_surface: semantics of dsv2hip_enc_batch (bufs: 4 slots per stream, packets identical to dsv_enc on the same
 * pixels, 0, or -1 with every nbufs[k] = 0 for a failed step).  Refused as a whole with -1 -- before any encoder, frame counter,
 * device buffer or nbufs entry is touched -- for n <= 0, a NULL array, an unusable encoder, encoders of different geometry, a layout
 * that is neither value, a NULL plane[0] or plane[1] (PLANAR: or plane[2]), a pitch smaller than its row's bytes, or an encoder
 * with dsv2hip_enc_set_uyvy_input on.  The encoders stay usable.
 * dsv2hip_enc_surface_frame: the same for one encoder (dsv2hip_enc_device_frame); returns the packet count, 0 where the batch call
 * would return -1.
 * dsv2hip_enc_surface_stats: out2[0] / out2[1] = lockstep steps of this process whose surface ingest ran in the fast / in the
 * general form so far; reset != 0 clears the counts afterwards. */
enum { DSV2HIP_SURFACE_PLANAR = 0, DSV2HIP_SURFACE_SEMIPLANAR = 1 };
/* PACKED RGB SURFACES, converted on ingest -- what renderers, screen capture, image libraries and torch image tensors produce: four
 * bytes a pixel, no conversion kernel, planar intermediate or extra pass over memory on the caller's side.
 *   BGRA / RGBA: plane[0] = the picture, row y at plane[0] + y * pitch[0], w pixels of 4 bytes in the named byte order;
 *                pitch[0] >= 4 * w; plane[1..2] and pitch[1..2] are ignored; the alpha byte is ignored.
 * A valid RGB layout is DSV2HIP_SURFACE_BGRA or DSV2HIP_SURFACE_RGBA or-ed with any subset of DSV2HIP_CSC_BT709 |
 * DSV2HIP_CSC_FULL_RANGE (DSV2HIP_CSC_BT601 = 0 is the default matrix, limited range the default range); a CSC bit on PLANAR /
 * SEMIPLANAR, or any other value, is refused.  The layouts go through dsv2hip_enc_batch_surface and dsv2hip_enc_surface_frame and
 * everything said above holds for them: only read, only inside the rows, surf[k] copied, any alignment and pitch (16-byte aligned
 * pointers and pitches with w a multiple of 4 throughout the step's RGB surfaces take the fast form of the RGB ingest), layouts
 * mixed freely within one step -- packed, planar, NV12, BGRA-601, RGBA-709-full ... -- and a refused call touches nothing.  Refused
 * in addition: plane[0] == NULL, pitch[0] < 4 * w, an encoder with dsv2hip_enc_set_uyvy_input on.  The stream may have any of the five
 * chroma formats (4:4:4, 4:2:2, 4:2:0, 4:1:1, "4:1:0"); its format decides the subsampling of the conversion.
 *
 * THE CONVERSION (the contract: encoding an RGB surface gives exactly the packets dsv_enc gives on the planar picture it defines).
 * Integer arithmetic with 8-bit coefficients.  With N = 1 << (hs + vs), the pixels per chroma sample of the stream's format:
 *
 *   Y(x,y) = (yr*R + yg*G + yb*B + 128 + 256*ybase) >> 8
 *   U(cx,cy) = min(255, (SUM over the footprint of (ur*R + ug*G + ub*B) + N*32896) >> (8 + hs + vs))
 *   V likewise with vr, vg, vb
 *
 * The footprint of chroma sample (cx, cy) is the pixels (cx<<hs ... +(1<<hs)-1, cy<<vs ... +(1<<vs)-1), with coordinates clamped to
 * w-1 and h-1.  Edge pixels are repeated where cw or ch was rounded up.  This is a box average, with the chroma sample centred on
 * its footprint.  ybase is 16 for limited range and 0 for full range.
 *
 *   preset            yr  yg  yb    ur  ug  ub    vr   vg  vb
 *   BT601 (limited)   66 129  25   -38 -74 112   112  -94 -18
 *   BT709 (limited)   47 157  16   -26 -86 112   112 -102 -10
 *   BT601 | FULL      77 150  29   -43 -85 128   128 -107 -21
 *   BT709 | FULL      54 183  19   -29 -99 128   128 -116 -12
 *
 * Every chroma row sums to 0, so R = G = B gives U = V = 128; limited range yields Y 16 ... 235 and U, V 16 ... 240 without a clamp;
 * full range needs the min(255, ...) only for U and V at 128 * 255 (value 256), and Y reaches 255 exactly; every sum is non-negative
 * before the shift.
 * dsv2hip_enc_rgb_stats: out2[0] / out2[1] = lockstep steps of this process whose RGB ingest ran in the fast / in the general form
 * so far; reset != 0 clears the counts afterwards.  dsv2hip_enc_surface_stats keeps counting the steps' YUV surfaces only. */
enum { DSV2HIP_SURFACE_BGRA = 0x10,   /* bytes in memory: B G R A */
       DSV2HIP_SURFACE_RGBA = 0x11 }; /* bytes in memory: R G B A */
enum { DSV2HIP_CSC_BT601 = 0x000, DSV2HIP_CSC_BT709 = 0x100, DSV2HIP_CSC_FULL_RANGE = 0x200 }; /* or-ed into the layout of an RGB surface */
typedef struct dsv2hip_surface {
    const void *plane[3]; /* device memory. PLANAR: Y, U, V.  SEMIPLANAR: Y, interleaved UV (U first), plane[2] ignored.  BGRA / RGBA: the picture */
    size_t pitch[3];      /* bytes from one row to the next; pitch[2] ignored for SEMIPLANAR, pitch[1..2] for BGRA / RGBA */
    int layout;
} dsv2hip_surface;
int dsv2hip_enc_batch_surface(int n, DSV_ENCODER **encs, const dsv2hip_surface *surf, DSV_BUF *bufs, int *nbufs);
int dsv2hip_enc_surface_frame(DSV_ENCODER *enc, const dsv2hip_surface *surf, DSV_BUF *bufs);
void dsv2hip_enc_surface_stats(unsigned long long *out2, int reset);
void dsv2hip_enc_rgb_stats(unsigned long long *out2, int reset);
/* THREE-BYTE AND PLANAR RGB SURFACES, converted on ingest -- the image-side layouts that have no fourth byte: an OpenCV Mat (BGR24), a
 * PIL / numpy / torch uint8[h, w, 3] picture, and torch's own image convention uint8[3, h, w].  They are read in place: no kernel
 * on the caller's side that pads every pixel to four bytes or transposes the planes.
 *   BGR / RGB: plane[0] = the picture, row y at plane[0] + y * pitch[0], w pixels of 3 bytes in the named byte order;
 *              pitch[0] >= 3 * w; plane[1..2] and pitch[1..2] are ignored.
 *   RGBP:      plane[0] = R, plane[1] = G, plane[2] = B, each w bytes by h rows, one byte a sample, pitch[c] >= w for each, all three
 *              pointers non-NULL.  The planes are named by pointer: a tensor ordered B, G, R passes them in the other order (one
 *              layout value, not two).  A contiguous torch uint8[3, h, w] tensor is plane[c] = data_ptr + c * h * w, pitch[c] = w.
 * A valid layout is one of the three values or-ed with any subset of DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE, as BGRA / RGBA are;
 * any other bit, a DSV2HIP_SCALE_* value included, is refused.  The layouts go through dsv2hip_enc_batch_surface and
 * dsv2hip_enc_surface_frame, and everything said of in-surfaces above holds: only read, and only inside the rows (no byte of
 * padding, no byte behind the last row, no word that holds no byte of a row), surf[k] copied, any pointer alignment and any pitch,
 * layouts mixed freely within one step -- packed, NV12, BGRA, RGB, RGBP ... -- the stream in any of the five chroma formats, and a
 * refused call touches nothing.  Pointers and pitches that are multiples of 4 with w a multiple of 4, throughout the step's surfaces
 * of the kind (three-byte; planar), take the fast form of its ingest.
 * The conversion is THE CONVERSION above, character for character: a three-byte or planar picture gives exactly the packets that
 * the same pixels give as an RGBA surface with any alpha.
 * Refused: everything dsv2hip_enc_batch_surface refuses, a NULL plane the layout needs, pitch[0] < 3 * w (RGBP: any pitch[c] < w), an
 * encoder with dsv2hip_enc_set_uyvy_input on, a stream format outside the five.
 * Out of scope: the _scaled and _sized calls below refuse the three layouts altogether, also at the encoder's own size, and
 * dsv2hip_enc_scaled_dims / dsv2hip_enc_sized_dims return -1 for them; every decoder out-surface call, dsv2hip_dec_surface_dims and
 * dsv2hip_dec_sized_dims refuse them (delivery into these layouts is not done).
 * dsv2hip_enc_rgb3_stats: out4[0] / out4[1] = lockstep steps of this process whose three-byte ingest ran in the fast / in the general
 * form so far, out4[2] / out4[3] the same for planar RGB; reset != 0 clears the counts afterwards.  dsv2hip_enc_rgb_stats keeps
 * counting the steps' four-byte surfaces only, dsv2hip_enc_surface_stats their YUV surfaces only. */
enum { DSV2HIP_SURFACE_BGR = 0x20,    /* packed, bytes in memory: B G R, three bytes a pixel */
       DSV2HIP_SURFACE_RGB = 0x21,    /* packed, bytes in memory: R G B */
       DSV2HIP_SURFACE_RGBP = 0x22 }; /* planar: plane[0] = R, plane[1] = G, plane[2] = B, one byte a sample */
void dsv2hip_enc_rgb3_stats(unsigned long long *out4, int reset);
/* HALF, QUARTER AND EIGHTH-SIZE INGEST -- a proxy ladder (1080p + 540p + 270p) from ONE full-size surface of a renderer, a screen
 * capture, a hardware decoder or a torch image tensor: an encoder of W' x H' reads a surface that holds src_w x src_h with
 * W' = ceil(src_w / n), H' = ceil(src_h / n), and the picture is reduced in the ingest pass -- one read of the source, no full-size
 * planar picture in between, no resize kernel on the caller's side.  The counterpart of the decoder's half, quarter and eighth-size
 * delivery below, with the same values and ONE layout grammar for both directions.
 * surf[k].layout: any layout dsv2hip_enc_batch_surface takes, or-ed with at most one DSV2HIP_SCALE_* value; s = (layout >> 12) & 3
 * is the shift, n = 1 << s.  A scaled in-layout is valid exactly when it is a valid out-layout (below): PLANAR, SEMIPLANAR, BGRA /
 * RGBA with CSC bits, or-ed with at most one of the three values; every other bit is no layout (0x4000, 0x1012 ...), a CSC bit on
 * PLANAR / SEMIPLANAR is none, and 0x1010 is held back here too (half-size BGRA: 0x1110, 0x1210, 0x1310; BT.601 limited-range pixels
 * at half size: RGBA, 0x1011).
 * src_w[k] x src_h[k]: the size of the picture IN THE SURFACE (ceil is not invertible, so the caller says it).  The encoder's
 * vidmeta.width, .height must equal ceil(src_w / n), ceil(src_h / n).  The source planes are dsv_mk_frame's for src_w x src_h in the
 * encoder's chroma format, scw x sch the chroma size of THAT picture:
 *   PLANAR      {src_w, scw, scw} bytes by {src_h, sch, sch} rows
 *   SEMIPLANAR  {src_w, 2 * scw}  bytes by {src_h, sch}      rows
 *   BGRA / RGBA {4 * src_w}       bytes by {src_h}           rows
 * and every pitch must be at least its SOURCE row's bytes.  Nested round-ups commute, so reducing each source plane on its own gives
 * exactly the encoder's plane sizes.
 * dsv2hip_enc_batch_surface_scaled / dsv2hip_enc_surface_frame_scaled behave as dsv2hip_enc_batch_surface / _surface_frame in
 * everything else: one lockstep step, 4 DSV_BUF slots per stream, surf[k] copied, the surface only read and only inside its rows,
 * any pointer alignment and any pitch; the encoders of a step share a geometry, their surfaces may differ in layout, scale, source
 * size, pitch and alignment (a plain NV12 beside a quarter-size BGRA beside an eighth-size planar one).  With s = 0 the call does
 * exactly what the plain call does (src_w, src_h must then equal the encoder's).  The batch call refuses as a whole with -1, before
 * any encoder, counter, buffer or nbufs entry is touched, and the one-frame call returns 0, for: everything the plain calls refuse;
 * a NULL src_w / src_h array; a layout outside the grammar; src_w or src_h <= 0; a source whose reduction is not the encoder's
 * geometry; a pitch below the SOURCE row's bytes; a NULL plane the layout needs; an encoder with dsv2hip_enc_set_uyvy_input on; an RGB
 * layout on a format outside the five.  dsv2hip_enc_batch_surface and dsv2hip_enc_surface_frame keep refusing a layout with a scale.
 * dsv2hip_enc_scaled_dims: what an encoder of this source must be (enc_w, enc_h) and what the source planes are (row_bytes, rows;
 * entries a layout has no plane for are 0), for a chroma format `subsamp` (DSV_SUBSAMP_*): 0, or -1 for a NULL pointer, a layout
 * outside the grammar, a size <= 0, a format that is none of DSV_SUBSAMP_* (an RGB layout: of the five).
 *
 * THE CONTRACT (the packets are exactly dsv_enc's on the planar W' x H' picture defined here).
 * YUV surfaces: the decoder's REDUCTION (below) applied to each SOURCE plane P, pw x ph, on its own:
 *
 *   out(x, y) = ( SUM j<n, i<n  P(min(x*n + i, pw-1), min(y*n + j, ph-1))  +  (1 << (2*s - 1)) ) >> (2*s)
 *
 * SEMIPLANAR: the reduced U and V of the de-interleaved plane.  So a picture decoded at full size into a surface and encoded through
 * the scaled call gives the packets of the same picture decoded at that scale and encoded through the plain call.
 * RGB surfaces: THE CONVERSION above with every footprint enlarged by the scale and ONE rounding per sample:
 *
 *   Y'(x,y)   = ( SUM over n x n of (yr*R + yg*G + yb*B)  +  ((128 + 256*ybase) << 2s) ) >> (8 + 2s)
 *   U'(cx,cy) = min(255, ( SUM over (n << hs) x (n << vs) of (ur*R + ug*G + ub*B)  +  (32896 << (hs + vs + 2s)) ) >> (8 + hs + vs + 2s))
 *   V' likewise with vr, vg, vb
 *
 * The footprints start at (x*n, y*n) and (cx << (hs + s), cy << (vs + s)), with coordinates clamped to src_w-1 and src_h-1 -- one
 * clamp, on source coordinates.  The matrices are those of the table above.  For U and V this is the plain formula with hs + s, vs + s
 * in place of hs, vs; with s = 0 the whole is the plain conversion.  (Converting at full size and reducing, or reducing RGB and
 * converting, would round two or three times.)  A footprint of equal pixels gives what one pixel gives; limited range stays within
 * Y 16 ... 235 and U, V 16 ... 240 without a clamp; every sum is non-negative before its shift; the largest accumulator is 1024 pixels
 * x 255 x 128 = 33 423 360, so plain 32-bit sums suffice (tests/test_ingest_scale_cpu.py, over all 2^24 colours).
 * dsv2hip_enc_scale_stats: out4[0] / out4[1] = lockstep steps of this process whose scaled YUV ingest ran in the wide form (every
 * scaled YUV source plane of the step: pointer, pitch and SOURCE row bytes multiples of 16) / in the general form; out4[2] / out4[3]
 * = the same for the scaled RGB ingest (every scaled RGB surface of the step: pointer and pitch multiples of 16, src_w of 4).
 * reset != 0 clears the counts afterwards.  dsv2hip_enc_surface_stats and dsv2hip_enc_rgb_stats keep counting the steps' unscaled
 * surfaces only. */
int  dsv2hip_enc_batch_surface_scaled(int n, DSV_ENCODER **encs, const dsv2hip_surface *surf,
                                      const int *src_w, const int *src_h, DSV_BUF *bufs, int *nbufs);
int  dsv2hip_enc_surface_frame_scaled(DSV_ENCODER *enc, const dsv2hip_surface *surf, int src_w, int src_h, DSV_BUF *bufs);
int  dsv2hip_enc_scaled_dims(int src_w, int src_h, int subsamp, int layout, int *enc_w, int *enc_h,
                             size_t row_bytes[3], int rows[3]);
void dsv2hip_enc_scale_stats(unsigned long long *out4, int reset);
/* INGEST AT ANY LARGER SIZE -- a rendition ladder (720p, 480p, 360p, 224 x 224) from ONE 1080p surface: the mirror image of the
 * decoder's sized delivery below.  An encoder of W x H reads a surface that holds src_w[k] x src_h[k], and the picture is resampled to
 * W x H in the ingest pass by THE RESAMPLING defined at dsv2hip_dec_batch_surface_sized: the exact area average, one rounding.
 * An entry's meaning follows from its layout:
 *   - a layout with a DSV2HIP_SCALE_* value: the entry is exactly dsv2hip_enc_batch_surface_scaled's entry -- the same rule
 *     (W = ceil(src_w / n), H = ceil(src_h / n)), the same edge-repeating reduction, the same kernels, the same counters;
 *   - a layout without one: the entry is SIZED.  Any source with W <= src_w <= 8 W and H <= src_h <= 8 H is allowed, each axis on its
 *     own, anamorphic sizes included;
 *   - a sized entry with src_w = W and src_h = H is the plain ingest: it takes the plain path, must pass what the plain call asks,
 *     and counts in dsv2hip_enc_surface_stats / dsv2hip_enc_rgb_stats and in no resize statistic.
 * One step may hold plain, scaled and sized entries of any layouts side by side.  The source planes are dsv_mk_frame's for
 * src_w x src_h in the encoder's chroma format (scw x sch the chroma size of THAT picture), as for the scaled call:
 *   PLANAR      {src_w, scw, scw} bytes by {src_h, sch, sch} rows
 *   SEMIPLANAR  {src_w, 2 * scw}  bytes by {src_h, sch}      rows
 *   BGRA / RGBA {4 * src_w}       bytes by {src_h}           rows
 * and every pitch must be at least its SOURCE row's bytes.  dsv2hip_enc_sized_dims reports these planes for an encoder of
 * enc_w x enc_h: 0, or -1 for exactly what the batch call would refuse about sizes, layout or format (and for a NULL pointer).
 *
 * THE CONTRACT (the packets are exactly dsv_enc's on the planar W x H picture defined here).
 * YUV surfaces: each SOURCE plane P, pw x ph, is resampled on its own to the encoder's plane ow x oh (luma W x H, chroma cw x ch):
 * with pw / ow = a / b and ph / oh = c / d in lowest terms, D = a * c and wx, wy the overlap lengths of the resampling,
 *
 *   out(x, y) = ( SUM j SUM i  wy(y,j) * wx(x,i) * P(i, j)  +  floor(D / 2) ) / D
 *
 * SEMIPLANAR: the de-interleaved U and V planes are resampled.  The bounds are the resampling's, per plane: D <= 2^24, sides
 * <= 32 768.  No coordinate outside the plane exists in the formula, and none is read.  So a picture decoded at full size into a surface
 * and encoded through the sized call gives the packets of the same picture decoded at that size (dsv2hip_dec_batch_surface_sized,
 * PLANAR) and encoded through the plain call; and where src = n * enc for n = 2, 4, 8 the result equals the scaled call's.
 * RGB surfaces: ONE rounding per sample -- the packed picture is resampled as RGB and the matrix is applied to the weighted sums.
 * Let w(x,y; i,j) = wy * wx for src_w x src_h -> ow x oh, where ow x oh = W x H for luma (D) and = cw x ch, the encoder's chroma
 * plane, for chroma (Dc; a ratio of up to 32 per axis).  With S_R = SUM w * R, S_G, S_B and the rows and ybase of the table above:
 *
 *   Y'(x,y)   = ( yr*S_R + yg*S_G + yb*S_B + (128 + 256*ybase) * D ) / (256 * D)
 *   U'(cx,cy) = min(255, ( ur*S_R + ug*S_G + ub*S_B + 32896 * Dc ) / (256 * Dc) )
 *   V' likewise with vr, vg, vb
 *
 * Where src = n * enc and W, H are multiples of the chroma subsampling this is exactly the scaled call's formula.  A footprint of
 * equal pixels gives what one pixel gives (the weights of a sample add up to D).  Every numerator is non-negative: the weights are,
 * and a chroma row's negative coefficients times 255 stay below 32 896.  For every plane of an RGB source the call requires
 * D <= 65 535 (Dc likewise) in addition: the weights of a sample add up to D, so a channel sum is at most 255 * D, a matrix row's
 * positive part at most 128 * 255 * D (luma: 256 * 255 * D less what the bias takes: the largest luma numerator of the four presets is
 * 65 408 * D), and with the bias every numerator is at most 65 536 * D, which fits 32 bits exactly when D <= 65 535; the divisor
 * 256 * D is then below 2^24 (tests/test_ingest_resize_cpu.py checks both over the extreme colours of all four presets).
 * 1920 x 1080 -> 1280 x 720 (D = 9, Dc = 9), 854 x 480 (D = 8 640, Dc = 17 280 at 4:2:0) and 224 x 224 (D = 8 100, Dc = 16 200) all pass
 * this bound (224 x 224 is taken from a source of up to 1792 wide: 1920 > 8 * 224 is outside the ratio, for YUV and RGB alike).
 * 1920 x 1080 -> 1918 x 1078 (D = 960 * 540 = 518 400) is refused for an RGB source and passes for a YUV one.
 * REFUSALS.  The batch call returns -1 before any encoder, counter, buffer or nbufs entry is touched, and the one-frame call returns
 * 0, for: everything the scaled call refuses; a sized entry outside the bounds above, per plane; src_w or src_h <= 0.
 * dsv2hip_enc_batch_surface, dsv2hip_enc_surface_frame and the scaled calls are unchanged: the scaled call with s = 0 and a source
 * size that is not the encoder's stays refused.
 * dsv2hip_enc_resize_stats: out4[0] / out4[1] = lockstep steps of this process whose sized YUV ingest ran in the wide form (every
 * sized YUV source plane of the step: pointer, pitch and SOURCE row bytes multiples of 4) / in the general form; out4[2] / out4[3] =
 * the same for the sized RGB ingest (every sized RGB surface of the step: pointer and pitch multiples of 4).  Sized entries count
 * here only; scaled entries count in dsv2hip_enc_scale_stats, own-size entries in the plain surfaces' counters.  reset != 0 clears
 * the counts afterwards.
 * Out of scope: enlargement; filters other than the area average; three-byte and planar RGB at another size than the encoder's
 * (DSV2HIP_SURFACE_BGR / _RGB / _RGBP are the plain call's alone); 10-bit; host surfaces. */
int  dsv2hip_enc_batch_surface_sized(int n, DSV_ENCODER **encs, const dsv2hip_surface *surf,
                                     const int *src_w, const int *src_h, DSV_BUF *bufs, int *nbufs);
int  dsv2hip_enc_surface_frame_sized(DSV_ENCODER *enc, const dsv2hip_surface *surf, int src_w, int src_h, DSV_BUF *bufs);
int  dsv2hip_enc_sized_dims(int src_w, int src_h, int enc_w, int enc_h, int subsamp, int layout,
                            size_t row_bytes[3], int rows[3]);
void dsv2hip_enc_resize_stats(unsigned long long *out4, int reset);
/* the same step with the pictures in HOST memory, as dsv_enc (dsv_encoder.c:1430) receives them: host_planar[k] is
 * stream k's packed planar picture of this step.  host_next (NULL, or NULL entries, allowed) names the picture each
 * stream will bring to the NEXT call: it is uploaded on a copy stream under this step's kernels, and the next call
 * finds it in HBM when it passes the same pointer as host_planar[k] (the bytes must not change in between).  With
 * pictures in pinned memory (dsv2hip_host_alloc) every upload is asynchronous.  This is the entry point bench.py
 * times: the host-to-device transfer of every frame is inside the measured region. */
int dsv2hip_enc_batch_host(int n, DSV_ENCODER **encs, const void *const *host_planar, const void *const *host_next,
                           DSV_BUF *bufs, int *nbufs);
/* frame ingest / egress on the GPU.  (a) Packed pictures given to this encoder are interleaved UYVY
 * 4:2:2 rows: the de-interleave that dsv_yuv_read does on the host (dsv.c:177-205) happens in the ingest kernel;
 * the metadata must say DSV_SUBSAMP_UYVY or DSV_SUBSAMP_422.  (b) Every picture this decoder returns is delivered
 * as 4:2:0: the chroma conversions of the reference CLI's -out420p (util.c:79-153: conv444to422 + conv422to420,
 * conv422to420, conv411to420, conv410to420; dsv_main.c:1030-1048) run on the GPU as the picture is written to the
 * output frame.  Both return 0, or -1 when the stream's format does not allow it. */
int dsv2hip_enc_set_uyvy_input(DSV_ENCODER *enc, int on);
int dsv2hip_dec_set_out420p(DSV_DECODER *dec, int on);
void *dsv2hip_host_alloc(size_t bytes); /* pinned host memory (NULL on failure) */
void dsv2hip_host_free(void *p);
/* lockstep decode over n independent decoder instances: packet bufs[k] goes to decs[k]; ret[k], out[k]
 * and fn[k] are exactly what dsv_dec(decs[k], &bufs[k], &out[k], &fn[k]) would have produced (packets are
 * consumed the same way).  All pictures of a step run through one set of kernel launches. */
int dsv2hip_dec_batch(int n, DSV_DECODER **decs, DSV_BUF *bufs, DSV_FRAME **out, DSV_FNUM *fn, int *ret);
/* Decoded pictures delivered to DEVICE memory (the mirror image of dsv2hip_enc_device_frame / dsv2hip_enc_batch: decode, processing
 * and encode can stay in HBM).
 * dsv2hip_dec_picture_bytes: bytes of one picture as this decoder delivers it to device memory: the packed planar layout
 * dsv2hip_enc_device_frame accepts (Y, U, V back to back, rows of exactly the plane's width, no padding; plane sizes as dsv_mk_frame
 * makes them), in the stream's format, or 4:2:0 when dsv2hip_dec_set_out420p is on.  0 before the decoder has seen metadata.
 * dsv2hip_dec_batch_device: dsv2hip_dec_batch without DSV_FRAMEs -- where dsv_dec would have returned a picture it is in dev_out[k]
 * (any alignment), complete when the call returns (the step's stream has drained: readable from any stream); ret[k], fn[k], the
 * packets' consumption and the decoders' state are those of dsv_dec (a picture was delivered where the decoder had metadata before
 * the call and ret[k] == DSV_DEC_OK); draw_info, out420p and postsharp are honoured as on the host
 * path.  Returns n, or -1 -- before any packet is touched or any decoder changed -- for n <= 0, a NULL array or decoder, or a decoder
 * that has metadata and whose dev_out[k] is NULL or dev_cap[k] < dsv2hip_dec_picture_bytes(decs[k]); a decoder without metadata
 * cannot yield a picture in the call and may pass NULL.
 * dsv2hip_dec_device_frame: the same for one decoder, as a step of its own (not through the dsv_dec submit queue); returns what
 * dsv_dec returns, or -1 (the packet untouched) where the batch call would return -1. */
size_t dsv2hip_dec_picture_bytes(DSV_DECODER *dec);
int dsv2hip_dec_batch_device(int n, DSV_DECODER **decs, DSV_BUF *bufs, void *const *dev_out, const size_t *dev_cap, DSV_FNUM *fn, int *ret);
int dsv2hip_dec_device_frame(DSV_DECODER *dec, DSV_BUF *buf, void *dev_out, size_t dev_cap, DSV_FNUM *fn);
/* Decoded pictures delivered into SURFACES with a row pitch in device memory -- what dsv2hip_enc_batch_surface reads, and what
 * hardware encoders, display paths, image libraries and hipMallocPitch work on: no repacking pass behind the decoder, and for the
 * semiplanar layouts (NV12 / NV16 / NV24) the chroma interleave happens on the way out.
 *   PLANAR:     plane[0..2] = Y, U, V, row y of plane c at plane[c] + y * pitch[c].
 *   SEMIPLANAR: plane[0] = Y, plane[1] = one interleaved chroma plane, rows of 2 * cw bytes U0 V0 U1 V1 ...; plane[2], pitch[2] and
 *               cap[2] are ignored.  Allowed for every chroma format.
 * The picture is the stream's format, or 4:2:0 when dsv2hip_dec_set_out420p is on (NV12 then: the conversion and the interleave
 * are one kernel, no planar 4:2:0 picture is written in between); plane sizes are dsv_mk_frame's: luma w x h, chroma cw x ch (the
 * format's shifts, rounded up).  Any pointer alignment and any pitch from the row's bytes up to INT_MAX is accepted; the surfaces
 * of one step may differ in layout, pitch and alignment.  Only bytes inside the rows are written: the padding between rows, the
 * bytes behind the last row and plane[2] of a semiplanar surface never are.  cap[c] is what the caller owns from plane[c] on.
 * Overlapping planes are the caller's error and are not checked.  A packed picture (dsv2hip_dec_batch_device) is the planar
 * surface with pitch = {w, cw, cw}: one code path serves both.
 * dsv2hip_dec_surface_dims: row bytes and row count of each plane of the picture as this decoder delivers it, for `layout`
 * (SEMIPLANAR: entry 1 = 2 * cw x ch, entry 2 = 0 x 0).  0, or -1 for a NULL decoder or array, a decoder that has seen no metadata
 * yet, or a layout that is neither value.
 * dsv2hip_dec_batch_surface: dsv2hip_dec_batch_device with surf[k] instead of a packed buffer -- ret[k], fn[k], the packets'
 * consumption and the decoders' state are those of dsv_dec; a picture is delivered exactly where the packed call would deliver one,
 * complete when the call returns; draw_info, out420p and postsharp are honoured as on every other delivery.  surf[k] is copied:
 * the array need not outlive the call.  Returns n, or -1 -- before any packet is touched or any decoder changed -- for n <= 0, a NULL
 * array or decoder, or a decoder that has metadata and whose surface has a layout that is neither value, a NULL plane[0] or plane[1]
 * (PLANAR: or plane[2]), a pitch smaller than its row's bytes (or beyond INT_MAX), or cap[c] < (rows[c] - 1) * pitch[c] +
 * row_bytes[c].  A decoder without metadata cannot yield a picture in the call: its entry may be all zeros.
 * dsv2hip_dec_surface_frame: the same for one decoder, as a step of its own; returns what dsv_dec returns, or -1 (the packet
 * untouched) where the batch call would return -1.
 * dsv2hip_dec_surface_stats: out2[0] / out2[1] = device rounds of this process (one per picture geometry present in a lockstep
 * step) whose chroma interleave ran in the wide form (every interleaved plane of the round: pointer and pitch multiples of 16,
 * cw of 8) / in the general form so far; rounds without a semiplanar picture count as neither.  reset != 0 clears the counts
 * afterwards.
 *
 * PACKED RGB SURFACES, converted on egress -- what display paths, image libraries and torch uint8[h, w, 4] tensors take: four bytes a
 * pixel, no conversion kernel and no second pass over memory behind the decoder.  The counterpart of the encoder's RGB surfaces
 * above, with the same constants and the same meaning.
 *   BGRA / RGBA: plane[0] = the picture, row y at plane[0] + y * pitch[0], w pixels of 4 bytes in the named byte order; the fourth
 *                byte of every pixel is written as 255; plane[1..2], pitch[1..2] and cap[1..2] are ignored.
 * A valid RGB layout is DSV2HIP_SURFACE_BGRA or DSV2HIP_SURFACE_RGBA or-ed with any subset of DSV2HIP_CSC_BT709 |
 * DSV2HIP_CSC_FULL_RANGE; a CSC bit on PLANAR / SEMIPLANAR, or any other value (0x12, 0x410 ...), is no layout.  The layouts go
 * through dsv2hip_dec_batch_surface and dsv2hip_dec_surface_frame, and everything said above holds for them, applied to plane 0: any
 * pointer alignment and any pitch from 4 * w up to INT_MAX; only the 4 * w bytes of each of the h rows are ever written, padding
 * and the bytes behind the last row never; cap[0] >= (h - 1) * pitch[0] + 4 * w; surf[k] copied; layouts mixed freely within one
 * step and one round -- packed, planar, NV12, BGRA-601, RGBA-709-full ...; a refused call touches nothing.  The stream may have any
 * of the five chroma formats.  Refused in addition -- as a whole, with -1, for a decoder that has metadata: an RGB layout on a decoder
 * with dsv2hip_dec_set_out420p on (an RGB picture has no chroma planes to subsample).  dsv2hip_dec_surface_dims gives row_bytes =
 * {4 * w, 0, 0} and rows = {h, 0, 0} for an RGB layout, and -1 for that pair too.
 *
 * THE CONVERSION (the contract: the delivered RGB picture is exactly this function of the planar picture that the same decoder,
 * with the same draw_info / postsharp settings, delivers through a PLANAR surface).  Integer arithmetic.  hs, vs are the stream's
 * chroma shifts; the chroma of pixel (x, y) is the sample (x >> hs, y >> vs): replication over exactly the footprint the encoder's
 * box average uses.  Bilinear or sited chroma upsampling is out of scope.
 *
 *   C = ky * (Y - ybase),  D = U - 128,  E = V - 128
 *   R = clamp((C + rv*E         + 128) >> 8, 0, 255)
 *   G = clamp((C + gu*D + gv*E  + 128) >> 8, 0, 255)
 *   B = clamp((C + bu*D         + 128) >> 8, 0, 255)      (>> arithmetic, i.e. floor)
 *
 *   preset            ky  ybase   rv    gu    gv    bu
 *   BT601 (limited)  298    16   409  -100  -208   516
 *   BT709 (limited)  298    16   459   -55  -136   541
 *   BT601 | FULL     256     0   359   -88  -183   454
 *   BT709 | FULL     256     0   403   -48  -120   475
 *
 * Over all 2^24 (Y, U, V): C + rv*E, C + gu*D + gv*E and C + bu*D lie within -74 016 ... 139 929 (with the rounding constant: -73 888
 * ... 140 057 at the shift), so 24-bit signed multiply-adds suffice;
 * U = V = 128 gives R = G = B; limited range maps Y = 16 to 0 and Y = 235 to 255; full range gives a grey Y back exactly.  Behind
 * the encoder's conversion at 4:4:4 (above) the round trip R, G, B -> Y, U, V -> R, G, B errs by at most 2, 2, 3 (R, G, B) with the
 * limited-range presets and 2, 1, 2 with the full-range ones, over all 2^24 colours (tests/test_egress_rgb_cpu.py).
 * draw_info and postsharp act on the luma the conversion reads, as they act on the luma plane of every other delivery.
 * dsv2hip_dec_rgb_stats: out2[0] / out2[1] = device rounds of this process whose RGB egress ran in the wide form (every RGB surface
 * of the round: pointer and pitch multiples of 16, w of 4) / in the general form so far; rounds without an RGB picture count as
 * neither.  reset != 0 clears the counts afterwards.  dsv2hip_dec_surface_stats keeps counting the chroma interleaves only.
 *
 * HALF, QUARTER AND EIGHTH-SIZE DELIVERY -- thumbnails, scrub strips, proxy renditions (decode 1080p, encode 540p and 270p from the
 * same step: dsv2hip_enc_batch_surface reads such surfaces in place), model input: the picture arrives at the consumer's size, without
 * a full-size write and read in between.  The scale belongs to the SURFACE: at most one of DSV2HIP_SCALE_HALF / _QUARTER / _EIGHTH
 * or-ed into the layout of an out surface, chosen per call and per picture; s = (layout >> 12) & 3 is the shift, n = 1 << s.  A
 * valid out-surface layout is any layout valid above (PLANAR, SEMIPLANAR, BGRA / RGBA with CSC bits) or-ed with at most one of the
 * three values; every other bit stays no layout (0x4000, 0x1012 ...).  ONE EXCEPTION: the value 0x1010 -- BGRA with the default
 * matrix and range at half size -- was documented and tested as "no layout" before the scale values existed, and stays refused by
 * all three calls; half-size BGRA is available with every other preset (0x1110, 0x1210, 0x1310), half-size BT.601 limited-range
 * pixels as RGBA (0x1011), and quarter and eighth size (0x2010, 0x3010) are not affected.  The scale goes through dsv2hip_dec_batch_surface,
 * dsv2hip_dec_surface_frame and dsv2hip_dec_surface_dims; dsv_dec, dsv2hip_dec_batch, dsv2hip_dec_batch_device,
 * dsv2hip_dec_device_frame and dsv2hip_dec_picture_bytes know nothing of it, and the encoder's plain surface calls refuse such a layout (dsv2hip_enc_batch_surface_scaled takes it).
 * Everything said of out surfaces above holds, applied to the reduced sizes: any pointer alignment, any pitch from the row's bytes
 * up to INT_MAX, cap[c] >= (rows[c] - 1) * pitch[c] + row_bytes[c], only bytes inside the rows written, surf[k] copied, layouts and
 * scales mixed freely within one step and one round (full-size NV12 beside quarter-size BGRA beside half-size planar), a refused
 * call touches nothing.
 * SIZES.  Each plane is reduced on its own: a plane of pw x ph becomes ow = (pw + n - 1) >> s by oh = (ph + n - 1) >> s.  Nested
 * round-ups commute, so the reduced picture has exactly dsv_mk_frame's plane sizes for W' = ceil(w / n), H' = ceil(h / n) in the
 * stream's format (chroma cw' x ch' by the format's shifts, rounded up) and can be handed to an encoder of that geometry.
 * dsv2hip_dec_surface_dims reports them: PLANAR {W', cw', cw'} by {H', ch', ch'}; SEMIPLANAR {W', 2 * cw', 0} by {H', ch', 0}; RGB
 * {4 * W', 0, 0} by {H', 0, 0}.
 * THE REDUCTION (the contract), for every plane P of the full-size picture:
 *
 *   out(x, y) = ( SUM j<n, i<n  P(min(x*n + i, pw-1), min(y*n + j, ph-1))  +  (1 << (2*s - 1)) ) >> (2*s)
 *
 * A box average with ONE rounding over the whole footprint (not an iterated pairwise one); a footprint that crosses the plane's right
 * or bottom edge repeats the edge pixel -- the footprint rule of the encoder's RGB ingest above.  The sum is at most 64 * 255 =
 * 16 320.  For s = 1 on a plane of even size this is the reference's dsv_ds2x_frame_luma (frame.c:211).
 * The delivered picture is this function of the picture that the same decoder, under the same draw_info and postsharp settings,
 * delivers through a full-size PLANAR surface: the overlay and the sharpening act on the full-size luma BEFORE the reduction (a
 * thumbnail of a drawn-on picture is the drawn-on picture reduced).  SEMIPLANAR: the interleave of the reduced U and V planes.  RGB:
 * THE CONVERSION above applied to the reduced planes -- pixel (x, y) of the reduced picture takes reduced chroma sample (x >> hs,
 * y >> vs).  The picture later P pictures predict from is never touched.  Other ratios: DELIVERY AT ANY SMALLER SIZE below; other filters are out of scope.
 * Refused in addition -- as a whole, with -1, for a decoder that has metadata: a scaled layout on a decoder with
 * dsv2hip_dec_set_out420p on (reducing behind the 4:2:0 conversion is out of scope, as RGB behind it is);
 * dsv2hip_dec_surface_dims returns -1 for that pair too.
 * dsv2hip_dec_scale_stats: out2[0] / out2[1] = device rounds of this process whose reduction ran in the wide form (every reduced
 * plane that goes straight into a caller's surface -- PLANAR: all three, SEMIPLANAR: luma -- has a pointer and a pitch that are
 * multiples of 8 and a reduced width that is a multiple of 16 >> s, i.e. of 8, 4, 2) / in the general form so far; rounds without a
 * scaled picture count as neither.  reset != 0 clears the counts afterwards.  The two other counters keep their meaning: a scaled
 * semiplanar or RGB picture's interleave / conversion counts there as any other. */
enum { DSV2HIP_SCALE_HALF = 0x1000, DSV2HIP_SCALE_QUARTER = 0x2000, DSV2HIP_SCALE_EIGHTH = 0x3000 }; /* or-ed into the layout of an OUT surface, or of an in surface of the _scaled calls */
typedef struct dsv2hip_out_surface {
    void *plane[3];  /* device memory. PLANAR: Y, U, V.  SEMIPLANAR: Y, interleaved UV (U first); plane[2] ignored.  BGRA / RGBA: the picture */
    size_t pitch[3]; /* bytes from one row to the next; pitch[2] ignored for SEMIPLANAR, pitch[1..2] for BGRA / RGBA */
    size_t cap[3];   /* bytes the caller owns from plane[c] on; cap[2] ignored for SEMIPLANAR, cap[1..2] for BGRA / RGBA */
    int layout;      /* DSV2HIP_SURFACE_PLANAR / _SEMIPLANAR, or DSV2HIP_SURFACE_BGRA / _RGBA or-ed with DSV2HIP_CSC_* bits; any of them or-ed
                        with at most one DSV2HIP_SCALE_* value */
} dsv2hip_out_surface;
int dsv2hip_dec_surface_dims(DSV_DECODER *dec, int layout, size_t row_bytes[3], int rows[3]);
int dsv2hip_dec_batch_surface(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_surface *surf, DSV_FNUM *fn, int *ret);
int dsv2hip_dec_surface_frame(DSV_DECODER *dec, DSV_BUF *buf, const dsv2hip_out_surface *surf, DSV_FNUM *fn);
void dsv2hip_dec_surface_stats(unsigned long long *out2, int reset);
void dsv2hip_dec_rgb_stats(unsigned long long *out2, int reset);
void dsv2hip_dec_scale_stats(unsigned long long *out2, int reset);
/* DELIVERY AT ANY SMALLER SIZE -- rendition ladders (1080p to 720p, 480p, 360p), model input (640 x 360, 224 x 224): the caller names
 * the delivered picture's size out_w x out_h, and every plane is resampled to it on the way out, without a full-size write and read
 * in between.  The size belongs to the CALL, per picture: dsv2hip_dec_batch_surface_sized is dsv2hip_dec_batch_surface with two more
 * arrays, dsv2hip_dec_surface_frame_sized its one-decoder form.  Semantics, ownership, return values, "surf[k] copied", "only bytes
 * inside the rows written", any pointer alignment, any pitch from the row's bytes up to INT_MAX, cap[c] >= (rows[c] - 1) * pitch[c] +
 * row_bytes[c] (with the sized rows, which dsv2hip_dec_sized_dims reports) and "a refused call touches nothing" are those of the
 * plain calls.  out_w[k] == 0 && out_h[k] == 0 means NOT SIZED: entry k behaves exactly as in the plain call, DSV2HIP_SCALE_* values in
 * its layout allowed, so one step -- and one device round -- may hold a full-size NV12 picture, a quarter-size BGRA picture and a 720p
 * planar picture side by side.  A sized entry's layout is a valid out-surface layout WITHOUT a scale value.
 * SIZES.  out_w <= w, out_h <= h, 8 * out_w >= w, 8 * out_h >= h: reduction only, down to an eighth, each axis on its own (anamorphic
 * sizes are allowed); the same bounds then hold for every chroma plane.  The delivered picture has exactly dsv_mk_frame's plane sizes
 * for out_w x out_h in the stream's format: chroma ocw = ceil(out_w >> hs) by och = ceil(out_h >> vs).  Each plane is resampled on
 * its own, pw x ph to ow x oh, by its own ratio; where the chroma ratio differs from the luma's (odd sizes) the chroma siting shifts
 * by a fraction of a sample, which is accepted.  dsv2hip_dec_sized_dims reports PLANAR {out_w, ocw, ocw} by {out_h, och, och};
 * SEMIPLANAR {out_w, 2 * ocw, 0} by {out_h, och, 0}; RGB {4 * out_w, 0, 0} by {out_h, 0, 0}; with out_w == out_h == 0 it is
 * dsv2hip_dec_surface_dims.
 * THE RESAMPLING (the contract) is an exact area average with one rounding, in integers.  Horizontally g = gcd(pw, ow), a = pw / g,
 * b = ow / g: source pixel i covers the interval [i*b, (i+1)*b), output sample x covers [x*a, (x+1)*a), and
 *   wx(x, i) = max(0, min((i+1)*b, (x+1)*a) - max(i*b, x*a))
 * is the length of their overlap; for every x the weights sum to exactly a.  Vertically the same with ph, oh: c = ph / gcd(ph, oh),
 * d = oh / gcd(ph, oh), wy(y, j) summing to c.  With D = a * c:
 *
 *   out(x, y) = ( SUM_j SUM_i  wy(y,j) * wx(x,i) * P(i, j)  +  floor(D / 2) )  /  D        (integer division, exact)
 *
 * - No coordinate outside the plane is ever read: the last sample's interval ends exactly at pw (pw * b = ow * a), so the formula
 *   knows no clamp and no edge repetition.
 * - Where pw = n * ow and ph = n * oh for n = 2, 4, 8 the result is exactly THE REDUCTION above (D = 4^s, rounding 1 << (2s - 1));
 *   with ow = pw, oh = ph it is the identity.
 * - Where the size is not divisible the two differ: DSV2HIP_SCALE_HALF on an odd width repeats the edge pixel in the last footprint,
 *   a sized delivery to ceil(w / 2) spreads the ratio pw / ow over the whole row.
 * - Constant planes stay constant.  A footprint spans at most 9 source pixels per axis (ratios up to 8).
 * - The sum is at most 255 * D + D / 2.  The call requires D <= 2^24 and every plane side <= 32 768 for every plane, so unsigned 32-bit
 *   sums suffice and x * a, i * b stay below 2^31; no plane of up to 4096 x 4096 comes near these limits (1919 x 1079 to 1279 x 719:
 *   D = 2 070 601).  1920 x 1080 to 1280 x 720 is a = c = 3, b = d = 2, D = 9: two taps per axis.
 * WHAT LEAVES, as with the scaled delivery: the picture is this function of the picture that the same decoder, under the same
 * draw_info and postsharp settings, delivers through a full-size PLANAR surface -- the overlay and the sharpening act on the
 * full-size luma first.  SEMIPLANAR: the interleave of the resampled U and V planes.  RGB: THE CONVERSION above applied to the
 * resampled planes.  The picture later P pictures predict from is never touched.  A sized entry with out_w == w and out_h == h
 * delivers exactly what the plain call delivers (it IS the plain delivery and counts in no resize statistic).
 * Refused as a whole with -1 (dsv2hip_dec_sized_dims: -1 as well): a NULL out_w / out_h array; for a decoder that has metadata:
 * exactly one of the two sizes zero, a negative size, a size outside the bounds above, D > 2^24 or a plane side > 32 768, a
 * DSV2HIP_SCALE_* value together with a size, a sized entry on a decoder with dsv2hip_dec_set_out420p on, and everything the plain
 * call refuses.  A decoder without metadata may pass anything, as before.
 * MEMORY: a sized SEMIPLANAR or RGB picture is resampled into a staging picture of the decoder's own, laid out at the planes' full
 * sizes on the first such picture (1.5 bytes a pixel for 4:2:0) and kept until the stream's geometry changes or the decoder is freed;
 * sized PLANAR delivery stages nothing.
 * Out of scope: enlargement; filters other than the area average; sized delivery behind out420p; three-byte and planar RGB out surfaces
 * (DSV2HIP_SURFACE_BGR / _RGB / _RGBP are refused by every out-surface call; planar RGB leaves through the tensor calls below); the host DSV_FRAME path (dsv_dec,
 * dsv2hip_dec_batch, dsv2hip_dec_batch_device know nothing of a size).  (The encoder's side: dsv2hip_enc_batch_surface_sized, above.)
 * dsv2hip_dec_resize_stats: out2[0] / out2[1] = device rounds of this process whose resampling ran in the wide form (every resampled
 * plane that goes straight into a caller's surface -- PLANAR: all three, SEMIPLANAR: luma -- has a pointer and a pitch that are
 * multiples of 4 and a width that is a multiple of 4: the kernel stores four samples as one dword) / in the general form so far;
 * rounds without a sized picture count as neither.  reset != 0 clears the counts afterwards.  A round's sized pictures count here
 * only, not in dsv2hip_dec_scale_stats; their interleave / conversion counts in the two other counters as any other picture's. */
int dsv2hip_dec_sized_dims(DSV_DECODER *dec, int layout, int out_w, int out_h, size_t row_bytes[3], int rows[3]);
int dsv2hip_dec_batch_surface_sized(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_surface *surf, const int *out_w, const int *out_h,
                                    DSV_FNUM *fn, int *ret);
int dsv2hip_dec_surface_frame_sized(DSV_DECODER *dec, DSV_BUF *buf, const dsv2hip_out_surface *surf, int out_w, int out_h, DSV_FNUM *fn);
void dsv2hip_dec_resize_stats(unsigned long long *out2, int reset);
/* PLANAR RGB TENSORS, u8 / f16 / bf16 / f32 -- what a vision model reads: [3, h, w], one plane per channel, usually floating point,
 * usually normalised per channel.  The picture leaves the decoder in that form, full size or at any smaller size, without a four-byte
 * surface and a second kernel of the caller's (drop alpha, transpose, convert, normalise) in between.  The out-surface calls keep
 * refusing the layouts 0x20 .. 0x22: a tensor has an element type and per-channel constants, which dsv2hip_out_surface has no room
 * for, so it has a descriptor and entry points of its own, and these serve the uint8 planar case too (what the encoder reads in place
 * as DSV2HIP_SURFACE_RGBP).
 * A contiguous torch [3, h, w] tensor is plane[c] = data_ptr + c * h * w * elem, pitch[c] = w * elem; a batch [n, 3, h, w] is n
 * descriptors.  The planes are named by POINTER: plane[0] receives R, plane[1] G, plane[2] B, and a model trained on B, G, R passes
 * them in the other order (scale[c] / bias[c] belong to plane[c]).  Planes may lie anywhere, also in different allocations.
 * Semantics are those of dsv2hip_dec_batch_surface and dsv2hip_dec_batch_surface_sized: ret[k], fn[k], packet consumption and decoder
 * state are dsv_dec's; t[k] is copied; only the row_bytes of each of the rows of each plane are written -- padding, the bytes behind
 * the last row and anything else never are; a decoder without metadata may pass anything (its entry is not looked at); draw_info and
 * postsharp act on the full-size luma before everything else; one step may mix element types, sizes, presets, constants and stream
 * geometries; a refused call touches nothing: no packet, decoder, fn, ret or tensor.
 * SIZE.  out_w == 0 && out_h == 0: the picture's own size.  Else the rules of DELIVERY AT ANY SMALLER SIZE above (reduction only,
 * down to an eighth per axis, every plane within THE RESAMPLING's bounds); out_w == w && out_h == h is the plain delivery and counts
 * in no resize statistic.  dsv2hip_dec_tensor_dims reports row_bytes = out_w * elem and rows = out_h (one pair: the three planes are
 * alike; elem = 1, 2, 2, 4), or the picture's own size for 0 x 0, and -1 wherever the batch call would refuse for dtype, size or
 * decoder.
 * THE CONTRACT.  The bytes R, G, B of pixel (x, y) are THE CONVERSION of the decoder's RGB surfaces (above; csc: any subset of
 * DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE) applied to the planar picture the same decoder delivers under the same settings --
 * for a sized tensor, to the planes resampled by THE RESAMPLING.  A U8 tensor therefore holds exactly bytes 0, 1, 2 of the RGBA
 * surface of the same call; scale and bias are ignored for it and may hold anything.  For a float dtype plane c holds, for its byte v,
 *
 *   f = fl32( fl32( (float) v * scale[c] ) + bias[c] )
 *
 * two IEEE binary32 operations, each rounded to nearest even, NOT fused into one multiply-add.  F32 stores f; F16 stores f converted
 * to binary16, round to nearest even, subnormals kept, overflow to infinity; BF16 stores f converted to bfloat16, round to nearest
 * even: (bits + 0x7fff + ((bits >> 16) & 1)) >> 16.  numpy reproduces all of it bit for bit: v.astype(np.float32) * np.float32(s) +
 * np.float32(b), then .astype(np.float16).  torchvision's ToTensor + Normalize(mean, std) is scale = 1 / (255 * std), bias = -mean /
 * std, folded by the caller; THIS form is the contract, and torch's own two steps (divide by 255, subtract, divide) may differ from it
 * in the last bit.
 * Refused as a whole with -1, for a decoder that has metadata: an unknown dtype; a csc bit outside the two; a NULL plane; a plane
 * pointer or a pitch that is not a multiple of the element size; a pitch below the row's bytes or beyond INT_MAX; cap[c] <
 * (rows - 1) * pitch[c] + row_bytes; scale[c] or bias[c] not finite (float dtypes only); dsv2hip_dec_set_out420p on; exactly one of
 * out_w / out_h zero; a size dsv2hip_dec_sized_dims refuses for an RGB layout.
 * MEMORY: as an RGB surface's -- a drawn-on or sharpened picture stages its luma, a sized one its resampled planes.
 * Out of scope: interleaved [h, w, 3] out tensors (they have the calls of INTERLEAVED RGB TENSORS below); the DSV2HIP_SCALE_* presets (a size covers them where it divides; THE RESAMPLING
 * says where the two differ); tensors and surfaces in one step; enlargement; any change to what the surface calls accept.
 * dsv2hip_dec_tensor_stats: out2[0] / out2[1] = device rounds of this process whose tensor conversion ran in the wide form (every
 * plane pointer and pitch of every tensor of the round a multiple of four elements and the delivered width a multiple of 4 -- any
 * contiguous torch tensor with w % 4 == 0: a thread's four samples of a row leave as one 4 / 8 / 16-byte store) / in the general form
 * so far; reset != 0 clears the counts afterwards.  Sized tensors also count in dsv2hip_dec_resize_stats, as any sized picture;
 * nothing counts in dsv2hip_dec_rgb_stats. */
enum { DSV2HIP_TENSOR_U8 = 0, DSV2HIP_TENSOR_F16 = 1, DSV2HIP_TENSOR_BF16 = 2, DSV2HIP_TENSOR_F32 = 3 };
typedef struct dsv2hip_out_tensor {
    void  *plane[3];   /* device memory: the R, G and B planes, named by pointer */
    size_t pitch[3];   /* bytes from one row to the next */
    size_t cap[3];     /* bytes the caller owns from plane[c] on */
    int    dtype;      /* DSV2HIP_TENSOR_* */
    int    csc;        /* any subset of DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE */
    int    out_w, out_h; /* 0, 0: the picture's own size; else the rules of DELIVERY AT ANY SMALLER SIZE */
    float  scale[3], bias[3]; /* for plane[c]; ignored (may hold anything) for U8 */
} dsv2hip_out_tensor;
int  dsv2hip_dec_tensor_dims(DSV_DECODER *dec, int dtype, int out_w, int out_h, size_t *row_bytes, int *rows);
int  dsv2hip_dec_batch_tensor(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_tensor *t, DSV_FNUM *fn, int *ret);
int  dsv2hip_dec_tensor_frame(DSV_DECODER *dec, DSV_BUF *buf, const dsv2hip_out_tensor *t, DSV_FNUM *fn);
void dsv2hip_dec_tensor_stats(unsigned long long *out2, int reset);
/* INTERLEAVED RGB TENSORS, u8 / f16 / bf16 / f32 -- what most image consumers take: an OpenCV Mat / GpuMat (BGR24), numpy, PIL, TF and
 * JAX pictures (uint8[h, w, 3], float NHWC), torch's channels_last memory format ([n, 3, h, w] that is [n, h, w, 3] in memory).  The
 * picture leaves the decoder with three elements a pixel, full size or at any smaller size, without a four-byte surface or a planar
 * tensor and a second pass of the caller's (drop alpha, permute) in between.  The out-surface calls keep refusing 0x20 / 0x21 and
 * dsv2hip_out_tensor has no layout field, so the interleaved tensor has a descriptor and entry points of its own.
 * A contiguous torch [h, w, 3] tensor, or a channels_last [1, 3, h, w] one, is data = data_ptr, pitch = 3 * w * elem; an OpenCV
 * GpuMat of CV_8UC3 is data = mat.data, pitch = mat.step, order DSV2HIP_SURFACE_BGR.
 * Semantics are those of dsv2hip_dec_batch_tensor: ret[k], fn[k], packet consumption and decoder state are dsv_dec's; t[k] is copied;
 * only the row_bytes = 3 * out_w * elem of each of the rows are written -- padding, the bytes behind the last row and anything else
 * never are; a decoder without metadata may pass anything (its entry is not looked at); draw_info and postsharp act on the full-size
 * luma before everything else; one step may mix element types, orders, sizes, presets, constants and stream geometries; a refused call
 * touches nothing: no packet, decoder, fn, ret or tensor.
 * SIZE.  As the planar tensor's: out_w == 0 && out_h == 0 is the picture's own size, else the rules of DELIVERY AT ANY SMALLER SIZE;
 * out_w == w && out_h == h is the plain delivery and counts in no resize statistic.  dsv2hip_dec_hwc_dims reports row_bytes =
 * 3 * out_w * elem and rows = out_h (the picture's own size for 0 x 0), and -1 wherever the batch call would refuse for dtype, size or
 * decoder.
 * THE CONTRACT.  The bytes R, G, B of pixel (x, y) are THE CONVERSION (csc: any subset of DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE)
 * of the planar picture the same decoder delivers under the same draw_info / postsharp settings -- for a sized tensor, of the planes
 * resampled by THE RESAMPLING.  Element k of a pixel is the channel `order` puts there: DSV2HIP_SURFACE_RGB R, G, B;
 * DSV2HIP_SURFACE_BGR B, G, R.  A U8 tensor in BGR order therefore holds exactly bytes 0, 1, 2 of the BGRA surface of the same call,
 * one in RGB order those of the RGBA surface; scale and bias are ignored for it and may hold anything.  For a float dtype element k of
 * every pixel holds, for its byte v, f = fl32( fl32( (float) v * scale[k] ) + bias[k] ), not fused, rounded to F16 / BF16 exactly as
 * the planar tensor's elements are.  The constants belong to MEMORY POSITIONS: a BGR consumer with ImageNet's constants passes them
 * in B, G, R order.
 * Refused as a whole with -1, for a decoder that has metadata: an unknown dtype; an order that is not exactly DSV2HIP_SURFACE_RGB or
 * DSV2HIP_SURFACE_BGR (0x22, the four-byte layouts and CSC bits in `order` included); a csc bit outside the two; a NULL data; data or
 * pitch not a multiple of the element size; a pitch below row_bytes or beyond INT_MAX; cap < (rows - 1) * pitch + row_bytes; scale[k]
 * or bias[k] not finite (float dtypes only); dsv2hip_dec_set_out420p on; exactly one of out_w / out_h zero; a size
 * dsv2hip_dec_sized_dims refuses for an RGB layout.
 * MEMORY: as an RGB surface's -- a drawn-on or sharpened picture stages its luma, a sized one its resampled planes.
 * Out of scope: a fourth channel (the BGRA / RGBA surfaces are that); the DSV2HIP_SCALE_* presets (a size covers them where it
 * divides); interleaved tensors together with surfaces or planar tensors in one call; enlargement; out420p; host memory; any change to
 * what the surface or planar-tensor calls accept.  (The way back in: INTERLEAVED RGB FLOAT TENSORS AS ENCODER INPUT below.)
 * dsv2hip_dec_hwc_stats: out2[0] / out2[1] = device rounds of this process whose interleaved conversion ran in the wide form (data and
 * pitch of every interleaved tensor of the round multiples of four elements and the delivered width a multiple of 4 -- any contiguous
 * torch [h, w, 3] or channels_last [1, 3, h, w] tensor with w % 4 == 0: a thread's twelve elements of a row leave as whole vector
 * stores) / in the general form so far; reset != 0 clears the counts afterwards.  Sized tensors also count in
 * dsv2hip_dec_resize_stats, as any sized picture; nothing counts in dsv2hip_dec_rgb_stats or dsv2hip_dec_tensor_stats. */
typedef struct dsv2hip_out_hwc {
    void  *data;      /* device memory: pixel (x, y) at data + y * pitch + 3 * x * elem */
    size_t pitch;     /* bytes from one row to the next */
    size_t cap;       /* bytes the caller owns from data on */
    int    dtype;     /* DSV2HIP_TENSOR_* (the planar tensor's enum, reused) */
    int    order;     /* DSV2HIP_SURFACE_RGB: elements R G B;  DSV2HIP_SURFACE_BGR: B G R */
    int    csc;       /* any subset of DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE */
    int    out_w, out_h;          /* 0, 0: the picture's own size; else DELIVERY AT ANY SMALLER SIZE */
    float  scale[3], bias[3];     /* for ELEMENT k of every pixel, in memory order; ignored for U8 */
} dsv2hip_out_hwc;
int  dsv2hip_dec_hwc_dims(DSV_DECODER *dec, int dtype, int out_w, int out_h, size_t *row_bytes, int *rows);
int  dsv2hip_dec_batch_hwc(int n, DSV_DECODER **decs, DSV_BUF *bufs, const dsv2hip_out_hwc *t, DSV_FNUM *fn, int *ret);
int  dsv2hip_dec_hwc_frame(DSV_DECODER *dec, DSV_BUF *buf, const dsv2hip_out_hwc *t, DSV_FNUM *fn);
void dsv2hip_dec_hwc_stats(unsigned long long *out2, int reset);
/* PLANAR RGB FLOAT TENSORS AS ENCODER INPUT, f16 / bf16 / f32 -- what a model or a renderer produces: a diffusion decoder, a
 * super-resolution network, a neural renderer, a simulator emit float [3, h, w] in device memory, usually normalised.  The encoder
 * reads it in place: no kernel of the caller's in front (de-normalise, clamp, round, store uint8[3, h, w]) whose rounding every
 * caller would pick for themselves.  The counterpart of the out-tensor calls above; the element types are their enum.
 * A contiguous torch [3, h, w] tensor is plane[c] = data_ptr + c * h * w * elem, pitch[c] = w * elem (elem = 2, 2, 4); a batch
 * [n, 3, h, w] is n descriptors.  The planes are named by POINTER: plane[0] is read as R, plane[1] as G, plane[2] as B, and a B-G-R
 * producer passes them in the other order (scale[c] / bias[c] belong to plane[c]).  Planes may lie anywhere, also in different
 * allocations.
 * Semantics are those of dsv2hip_enc_batch_surface / dsv2hip_enc_surface_frame: 4 buffer slots per stream, their return values, t[k]
 * copied by value (it may go once the call returns).  The tensor is only read, and only inside its rows -- no byte of padding, no byte
 * behind the last row; it is never written.  The picture has the encoder's size.  One step may mix element types, presets, constants,
 * tensor geometries (pointers, pitches, and so the form) and whatever else dsv2hip_enc_batch_surface lets the streams of a step
 * differ in; a refused call touches nothing: no encoder, buffer, nbufs or tensor.
 * THE CONTRACT.  For element e of plane c -- a binary16 or bfloat16 element widened EXACTLY to binary32 --
 *
 *   g = fl32( fl32( e * scale[c] ) + bias[c] )
 *   v = 0                              where g is a NaN
 *       rint( min( max(g, 0), 255 ) )  else, ties to even, as a byte
 *
 * g is two IEEE binary32 operations, each rounded to nearest even, NOT fused into one multiply-add.  So +inf gives 255, -inf and -0
 * give 0, a tie k + 0.5 goes to the even neighbour (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254, 255.5 -> 255).  Subnormal elements and
 * intermediates take part with their value: nothing is flushed to zero.  In numpy: np.rint(np.clip(g, 0, 255)) with g = e.astype(
 * np.float32) * np.float32(s) + np.float32(b), after replacing NaNs by 0.  The packets are exactly those of
 * dsv2hip_enc_batch_surface on a DSV2HIP_SURFACE_RGBP | csc surface that holds the bytes v: THE CONVERSION above, character for
 * character.
 * The inverse of the decoder's constants is scale' = 1 / scale, bias' = -bias / scale, folded by the caller; for torchvision's
 * ToTensor + Normalize(mean, std) that is scale' = 255 * std, bias' = 255 * mean.  ROUND TRIP: a byte delivered by
 * dsv2hip_dec_batch_tensor under scale = 1 / 255, bias = 0 or under the ImageNet constants (mean 0.485, 0.456, 0.406, std 0.229, 0.224,
 * 0.225) comes back as the same byte under these inverse constants, for F32, F16 and BF16 alike -- checked for all 256 bytes of every
 * channel (tests/test_ingest_tensor_cpu.py).  That is a checked fact about these constants, NOT a theorem: with other constants, a
 * BF16 or F16 element (8 or 11 significant bits) need not come back as the byte it was made from.
 * DSV2HIP_TENSOR_U8 is accepted and IS the planar RGB surface: the same records and kernel as DSV2HIP_SURFACE_RGBP | csc, scale and
 * bias ignored (they may hold anything); it counts in dsv2hip_enc_rgb3_stats, not in dsv2hip_enc_tensor_stats.
 * Refused as a whole (the batch call returns -1, the one-frame call 0 packets): everything dsv2hip_enc_batch_surface refuses for an
 * RGB layout (an encoder with dsv2hip_enc_set_uyvy_input on, a stream format outside the five, encoders of different step keys ...);
 * an unknown dtype; a csc bit outside the two; a NULL plane; a plane pointer or a pitch that is not a multiple of the element size; a
 * pitch below w * elem; a scale[c] or bias[c] that is not finite (float dtypes only).
 * Out of scope: interleaved [h, w, 3] float tensors (they have the calls of INTERLEAVED RGB FLOAT TENSORS AS ENCODER INPUT below); the scaled and the sized route (they remain the surface calls' own, as for
 * three-byte and planar RGB); tensors and surfaces in one call; 10-bit; host memory; any change to what the surface calls accept.
 * dsv2hip_enc_tensor_stats: out2[0] / out2[1] = lockstep steps of this process whose float tensor ingest ran in the wide form (every
 * plane pointer and pitch of every float tensor of the step a multiple of four elements and w a multiple of 4 -- any contiguous torch
 * tensor with w % 4 == 0: a thread's four elements of a row arrive as one 8 / 16-byte load) / in the general form so far; reset != 0
 * clears the counts afterwards. */
typedef struct dsv2hip_in_tensor {
    const void *plane[3];   /* device memory: the R, G and B planes, named by pointer */
    size_t pitch[3];        /* bytes from one row to the next */
    int    dtype;           /* DSV2HIP_TENSOR_* (the decoder's enum, reused) */
    int    csc;             /* any subset of DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE */
    float  scale[3], bias[3]; /* for plane[c]; ignored (may hold anything) for U8 */
} dsv2hip_in_tensor;
int  dsv2hip_enc_batch_tensor(int n, DSV_ENCODER **encs, const dsv2hip_in_tensor *t, DSV_BUF *bufs, int *nbufs);
int  dsv2hip_enc_tensor_frame(DSV_ENCODER *enc, const dsv2hip_in_tensor *t, DSV_BUF *bufs);
void dsv2hip_enc_tensor_stats(unsigned long long *out2, int reset);   /* steps in the wide / in the general form */
/* INTERLEAVED RGB FLOAT TENSORS AS ENCODER INPUT, f16 / bf16 / f32 -- a torch channels_last model output, a float NHWC picture from JAX
 * or TF, a renderer's RGB float framebuffer, an OpenCV GpuMat of CV_32FC3 / CV_16FC3, the decoder's own INTERLEAVED RGB TENSORS after a
 * model has touched them.  The encoder reads it in place: no permute(2, 0, 1).contiguous() of the caller's in front of the planar
 * tensor call, which is a second pass as large as the ingest.  The counterpart of dsv2hip_dec_batch_hwc; the vocabulary is
 * dsv2hip_out_hwc's, the element types are the tensors' enum.
 * A contiguous torch [h, w, 3] tensor is data = data_ptr, pitch = 3 * w * elem (elem = 2, 2, 4).  A channels_last [n, 3, h, w] tensor
 * is [n, h, w, 3] in memory: n descriptors, data = data_ptr + i * h * w * 3 * elem, pitch = 3 * w * elem.  An OpenCV GpuMat of
 * CV_32FC3 / CV_16FC3 is data = mat.data, pitch = mat.step, order DSV2HIP_SURFACE_BGR.  A crop is data at its first pixel under the
 * parent's pitch.
 * Semantics are those of dsv2hip_enc_batch_tensor / dsv2hip_enc_tensor_frame: 4 buffer slots per stream, their return values, t[k]
 * copied by value.  The tensor is only read, and only inside its rows -- the 3 * w elements of each of the h rows; no byte of padding,
 * no byte behind the last row; it is never written.  The picture has the encoder's size.  One step may mix element types, orders,
 * presets, constants and tensor geometries; a refused call touches nothing: no encoder, buffer, nbufs or tensor.
 * THE CONTRACT.  Element k (k = 0, 1, 2 in memory order) of pixel (x, y), widened EXACTLY to binary32, gives
 *
 *   g = fl32( fl32( e * scale[k] ) + bias[k] )
 *   v = 0                              where g is a NaN
 *       rint( min( max(g, 0), 255 ) )  else, ties to even, as a byte
 *
 * which is THE CONTRACT of the planar tensor word for word -- two binary32 operations, NOT fused, nothing flushed to zero -- with
 * constants that belong to MEMORY POSITIONS as dsv2hip_out_hwc's do: under DSV2HIP_SURFACE_BGR scale[0] / bias[0] are blue's.  The
 * packets are exactly those of dsv2hip_enc_batch_surface on a DSV2HIP_SURFACE_RGB | csc or DSV2HIP_SURFACE_BGR | csc surface that
 * holds the bytes v at the same positions; equivalently those of dsv2hip_enc_batch_tensor on the de-interleaved planes, with the
 * constants permuted by the order.
 * The inverse of the decoder's constants is scale'[k] = 1 / scale[k], bias'[k] = -bias[k] / scale[k] position by position; a BGR
 * consumer of torchvision's Normalize(mean, std) passes 255 * std and 255 * mean in B, G, R order.  ROUND TRIP: an element delivered by
 * dsv2hip_dec_batch_hwc under scale = 1 / 255, bias = 0 or under the ImageNet constants, in either order, comes back as the byte it
 * was made from under these inverse constants, for F32, F16 and BF16 alike -- checked for all 256 bytes at every position
 * (tests/test_ingest_hwc_cpu.py).  A checked fact about these constants, NOT a theorem, as for the planar tensor.
 * DSV2HIP_TENSOR_U8 is accepted and IS the three-byte surface: the same record and kernel as order | csc through
 * dsv2hip_enc_batch_surface, scale and bias ignored (they may hold anything); it counts in dsv2hip_enc_rgb3_stats, not in
 * dsv2hip_enc_hwc_stats.
 * Refused as a whole (the batch call returns -1, the one-frame call 0 packets): everything dsv2hip_enc_batch_tensor refuses for an
 * RGB layout (UYVY input on, a stream format outside the five, encoders of different step keys ...); an unknown dtype; an order that
 * is not exactly DSV2HIP_SURFACE_RGB or DSV2HIP_SURFACE_BGR (0x22, the four-byte layouts and CSC bits in `order` included); a csc bit
 * outside the two; a NULL data; data or pitch not a multiple of the element size; pitch / elem < 3 * w; a scale[k] or bias[k] that is
 * not finite (float dtypes only).
 * Out of scope: the scaled and the sized route; interleaved tensors together with surfaces or planar tensors in one call; a fourth
 * channel (the BGRA / RGBA surfaces are that); 10-bit; host memory; any change to what the other calls accept.
 * dsv2hip_enc_hwc_stats: out2[0] / out2[1] = lockstep steps of this process whose interleaved float ingest ran in the wide form (data
 * and pitch of every such tensor of the step multiples of four elements and w a multiple of 4 -- any contiguous torch [h, w, 3] or
 * channels_last tensor with w % 4 == 0: a thread's twelve elements of a row arrive as three 8 / 16-byte loads) / in the general form
 * so far; reset != 0 clears the counts afterwards. */
typedef struct dsv2hip_in_hwc {
    const void *data;   /* device memory: pixel (x, y) at data + y * pitch + 3 * x * elem */
    size_t pitch;       /* bytes from one row to the next */
    int    dtype;       /* DSV2HIP_TENSOR_* */
    int    order;       /* DSV2HIP_SURFACE_RGB: elements R G B;  DSV2HIP_SURFACE_BGR: B G R */
    int    csc;         /* any subset of DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE */
    float  scale[3], bias[3];  /* for ELEMENT k of every pixel, in memory order; ignored for U8 */
} dsv2hip_in_hwc;
int  dsv2hip_enc_batch_hwc(int n, DSV_ENCODER **encs, const dsv2hip_in_hwc *t, DSV_BUF *bufs, int *nbufs);
int  dsv2hip_enc_hwc_frame(DSV_ENCODER *enc, const dsv2hip_in_hwc *t, DSV_BUF *bufs);
void dsv2hip_enc_hwc_stats(unsigned long long *out2, int reset);      /* steps in the wide / in the general form */
/* -postsharp of the reference CLI (dsv_main.c:1058-1060, :1084-1089) inside the decoder: the luma of every picture handed out from
 * now on -- by dsv_dec, dsv2hip_dec_batch and the device deliveries alike -- has dsv_post_process (bmc.c:340) applied, last: behind
 * the 4:2:0 conversion and the draw_info overlay, as the CLI gets it by calling it on the frame dsv_dec returned.  Chroma and the
 * picture later P pictures predict from are untouched.  May be called on a zero-initialised decoder before the first packet.
 * 0 on success, -1 for a NULL decoder. */
int dsv2hip_dec_set_postsharp(DSV_DECODER *dec, int on);
/* where the decoder parses the plane sections of the pictures it is given from now on (hzcc.c:451-585): 0 on the host (fastest with
 * ~16 host cores per GPU), 1 P pictures on the device (one wavefront per section: ~1.4 host cores per GPU), 2 every picture on the
 * device; -1 (the default when DSV2_DEC_DEVICE_PARSE is unset): by the number of cores the process may use.  Returns the mode in force. */
int dsv2hip_dec_parse_mode(void);
int dsv2hip_dec_set_parse_mode(int mode); /* 0 / 1 / 2 as above, < 0: back to the default; for pictures handed over after the call */
/* Submit queue behind dsv_enc / dsv_dec.  The reference's interface is one synchronous call per frame
 * (dsv_encoder.h:190-199, dsv_decoder.h:54-61); its own parallel recipe is one encoder per process
 * (parallel_encode_yuv.sh:31-52).  Threads that each loop dsv_enc (or dsv_dec) on an instance of their own are run
 * TOGETHER: calls that arrive within a bounded window (10 % of the last step, 100 us .. 2 ms; DSV2_COALESCE_US) and agree
 * on the picture geometry share one lockstep step, each call still returning when its own frame is finished, with the
 * packets dsv_enc alone would have produced.  DSV2_COALESCE=0 turns the queue off.  The stats calls report what it did:
 * out4[0] calls, [1] lockstep steps they ran as, [2] largest step, [3] microseconds leaders waited for expected callers. */
void dsv2hip_enc_queue_stats(unsigned long long *out4, int reset);
void dsv2hip_dec_queue_stats(unsigned long long *out4, int reset);
/* Encoder instances size their symbol (compaction) lists by need -- HALF the picture's coefficients (at least 65 536 symbols), the worst
 * case at once for lossless streams -- and enlarge them when a picture has more symbols (its symbols are then worked out a second time
 * and coded on the host; the packets are the same).  Number of such enlargements in this process so far: a stream pays at most
 * one.  DSV2_COMPACT_CAP=<symbols> overrides the initial size. */
long dsv2hip_enc_list_growths(void);
/* The GPU entropy coder (csrc/entropy_gpu.hip) hands a picture to the host coder when it raises flag 1 (the adaptive Rice state left
 * the tabulated range), 2 (its section buffer is too small) or 4 (a chunk of 1 024 symbols of 2^24 bits or more), and has the bytes
 * fetched by a copy when it raises 8 (finished, but larger than the pinned mirror); the packets are the same.  Number of pictures of
 * this process -- of planes, for dsv_encode_plane on the device coder -- for which the coder ITSELF raised `flag` (1, 2, 4 or 8) so
 * far; the tests' forced fall-back (DSV2_GPU_ENTROPY_FORCE_FALLBACK) is not counted.  -1 for any other argument. */
long dsv2hip_enc_ent_flag_count(int flag);
/* Which entropy coder the stage seam's dsv_encode_plane (section 5) runs behind the quantiser: 0 (the default) the host coder of
 * csrc/entropy.cpp, 1 the encoder's GPU coder with the encoder's own fall-back rule -- the plane as plane fm->cur_plane of a picture
 * whose other planes are empty.  on < 0 changes nothing.  Returns the setting in force.  DSV2_SEAM_GPU_ENTROPY=1 makes 1 the setting a
 * process starts with.  (dsv_decode_plane follows
 * dsv2hip_dec_set_parse_mode: mode 2 parses every section on the device, mode 1 those of fm->isP pictures.  The seam has no packet
 * length, so the device path takes the section and the 8 bytes behind it for the packet: bs->start must be readable for 8 bytes
 * behind the section's end -- which the reference, and the host path, read too when a damaged section's last code overruns -- and
 * where a damaged section makes the parse run on further than that, the device parser reads zeros where the other two read the
 * caller's bytes.) */
int dsv2hip_seam_set_gpu_entropy(int on);
/* Test seam behind the motion search: queues `field` (nblocks = nblocks_h * nblocks_v records, copied) for the NEXT picture of
 * `enc` that is searched.  The search still runs; behind it, and before the controller's sums are taken (k_block_stats_b), the
 * field replaces the level-0 field in device memory and nintra / ndiff / eligible / total_err replace the search's own four sums
 * (intra_pct = nintra * 100 / nb, scblocks = ndiff * 100 / max(eligible, 1), avg_err = total_err / nb: hme.c:1825-1832, :2015) on
 * the device and on the host.  Everything behind that -- scene-change test, rate control, votes, side information, prediction --
 * is the production path on that field.  A legal record is one the reference's dsv_hme can store (tests/field_cases.py).
 * field == NULL drops a queued field.  0 on success, -1 for a NULL encoder or a block count that is not the encoder's.  An encoder
 * that has not coded a picture yet does not know its block count: a field queued then is taken as it is, and one of the wrong size
 * is dropped at the next searched picture with a line on stderr -- that picture is coded from the search's own field. */
int dsv2hip_seam_set_field(DSV_ENCODER *enc, const DSV_MV *field, int nblocks, int nintra, int ndiff, int eligible, unsigned total_err);
/* The side-information coder (csrc/sideinfo.hip) hands a P picture to the host coders when a sub-stream outgrows its image or a
 * code the 15-pair form of the exp-Golomb code; the packets are the same.  Number of P pictures of this process for which the
 * kernel ITSELF decided so; the tests' forced fall-back (DSV2_SIDE_FORCE_FALLBACK) is not counted. */
long dsv2hip_enc_side_flag_count(void);
/* Device allocations that did not fit their instance's one-block arena (the block's size is an estimate): 0 unless the estimate has
 * drifted from the allocations it stands for. */
long dsv2hip_arena_fallbacks(void);
/* Test hook: the NEXT lockstep step of this process fails on purpose -- how = 1: as a motion search that did not deliver its
 * counters (the search has drained), how = 2: as a search token that never came (ingest / pyramids still enqueued).  The
 * failed step drains its streams before its job tables go back to the pool, releases the callers' frames, marks its encoders
 * dead; dsv_enc returns 0, the batch calls return -1 with every nbufs[k] = 0 (tests/test_gpu_robustness.py). */
void dsv2hip_test_fail_next_step(int how);
/* Residency census of a `make census` build (csrc/prio.h): resident wavefront-time of every kernel site, measured inside the
 * kernels while the lockstep groups share the chip.  dsv2hip_census_read writes one text line per site that ran -- "<file> <line>
 * <ticks of the 100 MHz clock x wavefronts> <workgroups> <wavefronts>" -- and returns the bytes written; the product build
 * carries no census and returns 0. */
void dsv2hip_census_reset(void);
int dsv2hip_census_read(char *out, int cap);
/* stage timing with HIP events on the stream each lockstep step runs on.  May be switched on and
 * off at any time (resets the totals).  dsv2hip_prof_read fills 9 entries (ingest+pyramid, HME,
 * predict, fwd SBT, quant+compact, inv SBT, reconstruct+filters, extend, and -- inside HME -- the level-0
 * search launch alone, the dominant kernel): milliseconds of stage span,
 * kernel launches, and *frames = steps folded in; dsv2hip_prof_read_units: stream-frames each
 * stage processed (what the algorithmic byte counts of DESIGN.md are multiplied by). */
void dsv2hip_prof_enable(int on);
int dsv2hip_prof_read(double *ms, long long *launches, long long *frames);
int dsv2hip_prof_read_units(long long *units);

/* Device-resident transform benchmark/ops handle: a plane set kept in HBM. */
typedef struct dsv2hip_planeset dsv2hip_planeset;
/* allocate device buffers for one picture (format, width, height) and its coefficient planes */
dsv2hip_planeset *dsv2hip_planeset_create(int format, int width, int height);
void dsv2hip_planeset_destroy(dsv2hip_planeset *ps);
/* copy a host frame (planar, any stride) into the device picture / back */
int dsv2hip_planeset_upload(dsv2hip_planeset *ps, const DSV_FRAME *frame);
int dsv2hip_planeset_download(dsv2hip_planeset *ps, DSV_FRAME *frame);
int dsv2hip_planeset_set_blockdata(dsv2hip_planeset *ps, const uint8_t *blockdata, int nblocks_h, int nblocks_v);
/* run the forward / inverse transform of plane c entirely in HBM (asynchronous on the set's stream) */
int dsv2hip_planeset_fwd_sbt(dsv2hip_planeset *ps, int c, int isP, int lossless);
int dsv2hip_planeset_inv_sbt(dsv2hip_planeset *ps, int c, int q, int isP, int lossless);
int dsv2hip_planeset_get_coefs(dsv2hip_planeset *ps, int c, DSV_SBC *out);
int dsv2hip_planeset_set_coefs(dsv2hip_planeset *ps, int c, const DSV_SBC *in);
int dsv2hip_planeset_sync(dsv2hip_planeset *ps);
/* times `iters` back-to-back launches of one transform with HIP events on the set's stream;
 * returns the mean milliseconds per call (negative on error) */
float dsv2hip_planeset_time_sbt(dsv2hip_planeset *ps, int c, int isP, int lossless, int inverse, int q, int iters);

#ifdef __cplusplus
}
#endif
#endif
