/* yolov3_hip.h -- C ABI of libyolov3_hip.so (MI355X / gfx950 only).
 *
 * The reference (ultralytics/yolov3) is 100 % Python and has no FFI of its own:
 * every op on its detection hot path is an ATen call.  This header is the boundary a maintainer
 * binds instead of those ATen calls; each entry point names the reference call site it replaces.
 * The Python host side (yolov3_amd/) mirrors the reference's own signatures
 * (DetectionModel/Detect.forward, non_max_suppression, ComputeLoss) on top of these symbols.
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller (the host side
 *    allocates through torch's caching allocator so it is stream-ordered); no hidden hipMalloc,
 *    no host synchronisation inside any call; `stream` is a hipStream_t passed as void*.
 *  - activations are NHWC ("pixel-major"): element (n,h,w,c) at data[((n*H+h)*W+w)*pitch + c];
 *    `pitch` >= c lets a tensor be a channel slice of a wider buffer (zero-copy Concat).
 *  - return 0 on success, negative on error; y3_last_error() gives the thread-local message.
 */
#ifndef YOLOV3_HIP_H
#define YOLOV3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The Python binding (yolov3_amd/_header.py) is READ from this file: constants, struct layouts, every signature, and -- by the missing trailing `void* stream` -- the
 * exports that launch nothing.  Declare an export here, define it, write its ops wrapper; keep to the plain C the reader understands (it refuses the rest).
 * ABI history -- 2: tune / SyncBN / TTA / wgrad_plan added, y3_bn_act_bwd_apply takes sums + 2C; 3: y3_loss_params.sort_obj_iou;
 * 4: y3_conv_workspace_error / _reset removed (no-ops since the stream-K kernel went), the loss workspace grew by one int per slot;
 * 5: layer 0 by recomputation (three exports), y3_shard_mean, knob wgrad_patch;
 * 6: the deferred-epilogue form of conv_v10 and layer-0 recomputation removed. */
#define Y3_ABI_VERSION 6

typedef enum { Y3_F16 = 0, Y3_BF16 = 1, Y3_F32 = 2, Y3_U8 = 3 } y3_dtype;
typedef enum { Y3_ACT_NONE = 0, Y3_ACT_SILU = 1 } y3_act;
typedef enum { Y3_ALGO_AUTO = 0, Y3_ALGO_MFMA = 1, Y3_ALGO_DIRECT = 2 } y3_algo;

/* NHWC view. `data` already points at channel 0 of the slice. */
typedef struct {
    void* data;
    int32_t n, h, w, c;
    int32_t pitch; /* elements between consecutive pixels (>= c) */
} y3_tensor;

/* Fused Conv2d(k in {1,3}, stride in {1,2}, pad=k/2, groups=1) + bias + activation (+ residual).
 * Replaces reference models/common.py:75 / :81 (Conv.forward / forward_fuse: conv -> bn -> SiLU),
 * the residual add of models/common.py:165 (Bottleneck.forward), the nn.Upsample(x2, nearest) of
 * models/yolov3.yaml:43,51 (upsample2x != 0: every output pixel is written to its 2x2 block of the
 * (2*Ho, 2*Wo) destination) and torch.cat of models/common.py:428 (write into a channel slice). */
typedef struct {
    int32_t dtype;      /* y3_dtype of x / w / residual / y (F16, BF16, F32) */
    int32_t ksize;      /* 1 or 3 */
    int32_t stride;     /* 1 or 2 */
    int32_t act;        /* y3_act */
    int32_t upsample2x; /* 0 / 1 */
    int32_t algo;       /* y3_algo; AUTO = MFMA for F16/BF16, DIRECT for F32 */
    int32_t cin;        /* logical input channels of the packed filter (x->c must equal it) */
    int32_t cout;       /* output channels stored (multiple of 8; pad filters with zero rows) */
    int32_t in_dilation; /* 0/1 = plain; 2 = x is a virtual zero-interleaved (2h x 2w) image: data-gradient of a
                            stride-2 conv = stride-1 conv of the dilated output gradient with the flipped, transposed
                            filter (y3_pack_filter_dgrad); y's height/width then give the gradient's size */
    int64_t filter_elems; /* elements of `dtype` the caller's packed bank holds (ABI 4).  Non-zero: a bank shorter than y3_packed_filter_elems(cout, cin, ksize)
                             is refused -- e.g. one sized rows x Kpad by the ABI-1 rule, without the fragment-ordered second copy the persistent 3x3 kernel
                             reads behind the row-major one.  0 = unchecked: the caller vouches for the size */
} y3_conv_desc;

int y3_abi_version(void);
const char* y3_last_error(void);

/* Run-time tuning knobs: every A/B hook of the library in one table (no counterpart in the reference; ATen's equivalents are
 * torch.backends.cudnn.benchmark and friends).  Defaults are the measured-best settings.  Keys: "conv" (0 per-shape dispatch, 2 / 4 / 5 /
 * 6 / 15 force a tile variant), "conv_ahead" (3 / 2: K-steps the LDS-DMA requests run ahead), "bn_nt_bytes" (threshold of
 * the non-temporal BatchNorm passes), "wgrad" (0 per-shape, 2 128-tile, 3 256-tile, 4 direct fp32), "wgrad_xcd" (0..3), "dgrad_quad"
 * (1 / 0), "spp_direct" (0 / 1), "conv_v10" (1 auto, 0 off, 2 every eligible shape), "v10_mp" / "v10_blocks" (0 auto; widest wave tile / blocks per filter tile of csrc/conv_v10.h: tests), "v10_half" (2 auto, 0 one block per CU, 1 two half-size blocks per CU), "v10_ksplit" (1 small launches with a workspace, 0 never, 2 every eligible launch) / "v10_slices" (0 auto; forced slice count: tests), "v10_group" (1 the blocks of a filter tile on one XCD take the tiles of their common pixel range round-robin, 0 contiguous runs), "tile_xcd" (1 XCD-grouped tile ids in the persistent tile loops of csrc/stem.hip, 0 dispatch order), "conv_1x1s" (1 the persistent 1x1 kernel with register-resident filters of csrc/conv_1x1s.h on the HBM-bound 1x1 layers, 0 the tile kernels, 2 also small launches), "wgrad_strip" / "conv_strip" (1 the strip-walking kernels of csrc/wgrad_strip.h / conv_strip.h on the
 * small-channel 3x3 layers, 0 off, 2 also small launches, N > 2: N rows per block -- tests).  The environment variable Y3_TUNE="key=value,key=value" is read once when the library is first used.
 * Process-wide, not stream-ordered: set a knob before enqueueing the launches it should affect. */
int y3_tune_set(const char* key, int64_t value); /* 0, or -1 for an unknown key */
int64_t y3_tune_get(const char* key);            /* INT64_MIN for an unknown key */
void y3_tune_reset(void);                        /* defaults + Y3_TUNE again */

/* number of elements (of `dtype`) of a packed filter bank for (cout, cin, ksize).  ALWAYS size banks with this call: a 3x3 bank with cout % 256 == 0 and
 * cin % 32 == 0 is TWO copies -- the row-major one every kernel reads, followed by a fragment-ordered one (per 64-row wave and K-step a contiguous 4 KiB block
 * of four MFMA A fragments) that the persistent 3x3 kernel loads straight into registers (csrc/conv_v10.h, csrc/filter_bank.h::y3_frag_index).  Every packer
 * below (y3_pack_filter, _dgrad, _pair, _jobs) writes both (ABI version 2).  Every layout is defined in csrc/filter_bank.h, every packer lives in csrc/filter_bank.hip. */
size_t y3_packed_filter_elems(int32_t cout, int32_t cin, int32_t ksize);
/* OIHW fp32 (cout_src x cin_src x k x k) -> packed [cout_pad][k*k*cin_pad (+K pad)] in `dtype`;
 * `cout`/`cin` are the padded logical sizes used by y3_conv2d_fwd (>= the source sizes; pad = 0).
 * Replaces the layout the reference gets from nn.Conv2d.weight (models/common.py:68). */
int y3_pack_filter(const float* w_oihw, int32_t cout_src, int32_t cin_src, int32_t ksize, int32_t cout, int32_t cin,
                   int32_t dtype, void* packed, void* stream);

int y3_conv2d_fwd(const y3_conv_desc* desc, const y3_tensor* x, const void* packed_filter, const float* bias,
                  const y3_tensor* residual /* may be NULL */, const y3_tensor* y, void* stream);
/* The same call with a caller-owned scratch buffer of y3_conv_workspace_bytes() bytes (256-byte aligned, used by one stream at a time): unlocks the K-split
 * form of the persistent 3x3 kernel for SMALL launches of the 3x3 / stride-1 layers with cout % 256 == 0 (models/common.py:150-165 Bottleneck.cv2, the 3x3
 * convs of the head; batch 1-4 at 640x640) -- the channel blocks of every tile are cut into slices, every (tile, slice) writes fp32 partial sums into the
 * workspace and a second launch adds them in slice order and applies bias / SiLU / residual / statistics.  Results are deterministic (fixed split, fixed
 * summation order).  Launches the form does not cover run exactly as y3_conv2d_fwd. */
size_t y3_conv_workspace_bytes(void);
int y3_conv2d_fwd_ws(const y3_conv_desc* desc, const y3_tensor* x, const void* packed_filter, const float* bias,
                     const y3_tensor* residual /* may be NULL */, const y3_tensor* y, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Which kernel variant the dispatcher picks for this problem ("v10", "v10h", "v10k", "s1x1", "v6", "v3_bk64_128x128", "strip", ..., "direct"); launches nothing.
 * The parity tests assert it so that a tolerance is always attached to the kernel that actually ran. */
int y3_conv2d_fwd_variant(const y3_conv_desc* desc, const y3_tensor* x, const y3_tensor* y, int32_t has_residual,
                          size_t workspace_bytes, char* name, size_t name_capacity);
/* The tile plan of the persistent 3x3 kernel (csrc/conv_v10.h: "v10", "v10h", "v10k") for this problem; launches nothing.  One record of four int32 per tile of ONE filter
 * tile -- (block of the filter tile, tile of that block, first 32-pixel column block, column blocks) -- computed by the functions the kernel itself runs, so a host test can
 * check that the tiles cover the pixel axis exactly once and that the blocks sharing an XCD work on neighbouring tiles (knob "v10_group").  `records` may be NULL
 * (count only); *column_blocks = ceil(N Ho Wo / 32), *group_blocks = blocks per interleave group.  Fails when the dispatcher picks another kernel for the problem. */
int y3_conv_v10_tiles(const y3_conv_desc* desc, const y3_tensor* x, const y3_tensor* y, size_t workspace_bytes, int32_t* records,
                      int64_t capacity, int64_t* n_tiles, int32_t* column_blocks, int32_t* group_blocks);
/* Training forward of a 1x1 convolution whose INPUT is another layer's Conv + BatchNorm + activation (+ shortcut) output (reference models/common.py:75 Conv.forward inside
 * Bottleneck.forward, :165): `u_in` is that layer's pre-BatchNorm tensor; the launch computes y_in = act(in_scale * u_in + in_shift) (+ in_shortcut) on the way in -- the
 * arithmetic of y3_bn_act_fwd --, stores it to `y_in` once (the other consumers read it) and convolves it: y = conv1x1(y_in) + bias with statistics rows like
 * y3_conv2d_fwd_stats.  Replaces the y3_bn_act_fwd launch of the producing layer and this layer's read of y_in.  Only the HBM-bound Bottleneck.cv1 shapes
 * (cin / cout 64 / 32, 128 / 64, 256 / 128); y3_conv2d_fwd_bnin_rows returns the statistics rows, or -1 when the shape is not covered (the caller keeps the two launches). */
int64_t y3_conv2d_fwd_bnin_rows(const y3_conv_desc* desc, const y3_tensor* u_in, const y3_tensor* y_in, const y3_tensor* y, int32_t has_shortcut);
int y3_conv2d_fwd_bnin_stats(const y3_conv_desc* desc, const y3_tensor* u_in, const float* in_scale, const float* in_shift, int32_t in_act,
                             const y3_tensor* in_shortcut /* may be NULL */, const y3_tensor* y_in, const void* packed_filter, const float* bias, const y3_tensor* y,
                             float* stat_rows, int64_t capacity_rows, int64_t* n_rows, void* stream);
/* Name of the variant the last convolution / data-gradient call of the calling thread launched ("v3_quad": the four output-parity
 * classes of y3_conv2d_dgrad_s2 in one launch). */
int y3_conv_last_variant(char* name, size_t name_cap);

/* Stem convolution: the first layer `Conv(ch<=4, 32|64, 3, 1)` (reference models/yolov3.yaml:16, models/common.py:57-81) computed
 * straight from the caller's NCHW image, fused with the ingest (`im.half(); im /= 255`, val.py:354-360): no NHWC copy of the
 * image is made.  `packed` comes from y3_pack_filter_stem ([cout_pad32][3][16] in `dtype`, BN folded by the caller),
 * y is the NHWC output view (n, h, w, cout), stride 1 / pad 1 only; src_dtype u8 / f16 / bf16 / f32, compute f16 / bf16. */
size_t y3_packed_filter_stem_elems(int32_t cout);
int y3_pack_filter_stem(const float* w_oihw, int32_t cout_src, int32_t cin_src, int32_t cout, int32_t dtype, void* packed, void* stream);
int y3_stem_conv_fwd(const void* x_nchw, int32_t src_dtype, int32_t n, int32_t cin, int32_t h, int32_t w, float divisor, const void* packed,
                     const float* bias, int32_t dtype, int32_t act, const y3_tensor* y, void* stream);
/* Training form of the first layer (models/common.py:75 `act(bn(conv(x)))` with batch statistics): the same launch also writes one row
 * of (sum, sum of squares) per filter of the STORED values per block into stat_rows ([rows][y->c][2] floats; rows =
 * y3_stem_conv_stats_rows(n, h, w), reported in *n_rows) for y3_bn_finalize_rows -- no separate reduction pass over the output. */
int64_t y3_stem_conv_stats_rows(int32_t n, int32_t h, int32_t w);
int y3_stem_conv_fwd_stats(const void* x_nchw, int32_t src_dtype, int32_t n, int32_t cin, int32_t h, int32_t w, float divisor, const void* packed,
                           const float* bias, int32_t dtype, int32_t act, const y3_tensor* y, float* stat_rows, int64_t capacity_rows, int64_t* n_rows,
                           void* stream);
/* Layers 0 + 1 of yolov3 / yolov3-spp in one kernel (models/yolov3.yaml:16-17: Conv(3,32,3,1) -> Conv(32,64,3,2)): layer 0's
 * output (the largest tensor of the network, single consumer) stays in LDS.  packed0 / bias0: 32 filters in the stem format
 * (y3_pack_filter_stem); packed1 / bias1: 64 filters over 32 channels in the generic format (y3_pack_filter); y: NHWC
 * (n, (h-1)/2+1, (w-1)/2+1, 64). */
int y3_stem_pair_fwd(const void* x_nchw, int32_t src_dtype, int32_t n, int32_t cin, int32_t h, int32_t w, float divisor,
                     const void* packed0, const float* bias0, int32_t act0, const void* packed1, const float* bias1, int32_t act1,
                     int32_t dtype, const y3_tensor* y, void* stream);
/* Bottleneck(C, C), C = 64 or 128 (models/yolov3.yaml:18,20: layers 2 and 4) in one kernel: y = [x +] cv2(cv1(x)) with cv1 = 1x1 conv
 * C -> C/2 (+ bias1, act1) and cv2 = 3x3 stride-1 conv C/2 -> C (+ bias2, act2); the C/2-channel intermediate (rounded to the storage
 * dtype as the two-launch form stores it) stays in LDS and x is read once.  packed1 / packed2: generic banks (y3_pack_filter) of
 * C/2 x (1x1xC) and C x (3x3xC/2).  x, y: NHWC (n, h, w, C) views, not aliased. */
int y3_bneck_pair_fwd(const y3_tensor* x, const void* packed1, const float* bias1, int32_t act1, const void* packed2, const float* bias2,
                      int32_t act2, int32_t add_residual, int32_t dtype, const y3_tensor* y, void* stream);

/* NCHW (u8 / f16 / bf16 / f32) image batch -> NHWC `out_dtype`: cast, then true-divide by `divisor`
 * (1.0 = none) in the output dtype, channels zero-padded to out->c.
 * Replaces `im.half()/float(); im /= 255` of reference val.py:354-360 / train.py:380 when src is u8. */
int y3_nchw_to_nhwc(const void* src, int32_t src_dtype, int32_t n, int32_t c, int32_t h, int32_t w, float divisor,
                    int32_t out_dtype, const y3_tensor* out, void* stream);
/* NHWC -> contiguous NCHW of the same dtype (debug / feature export). */
int y3_nhwc_to_nchw(const y3_tensor* src, int32_t dtype, void* dst, void* stream);

/* MaxPool2d(k, stride, pad) with -inf padding; optional zero padding on the right/bottom edge first
 * (zpad_r, zpad_b) = nn.ZeroPad2d([0,zpad_r,0,zpad_b]).  Replaces reference models/yolov3-tiny.yaml:21-32
 * (nn.MaxPool2d / nn.ZeroPad2d) and one branch of SPP (models/common.py:287-290). */
int y3_maxpool2d(const y3_tensor* x, const y3_tensor* y, int32_t dtype, int32_t k, int32_t stride, int32_t pad,
                 int32_t zpad_r, int32_t zpad_b, void* stream);
/* SPP pyramid: y[..., c:2c]=mp5(x), [2c:3c]=mp9(x), [3c:4c]=mp13(x) in ONE pass; x may alias y[..., 0:c].
 * Replaces reference models/common.py:287-290 (3x max_pool2d + cat). */
int y3_spp_pyramid(const y3_tensor* x, const y3_tensor* y3c /* slice starting at channel c, 3c wide */, int32_t dtype,
                   void* stream);
/* nearest x2 upsample / channel-slice copy (fallbacks when not fused into a conv epilogue):
 * reference models/yolov3.yaml:43 (nn.Upsample) and models/common.py:428 (torch.cat). */
int y3_upsample2x(const y3_tensor* x, const y3_tensor* y, int32_t dtype, void* stream);
int y3_copy_slice(const y3_tensor* x, const y3_tensor* y, int32_t dtype, void* stream);

/* Detect head post-conv: reference models/yolo.py:98 (view/permute -> raw (bs,na,ny,nx,no)) and
 * :104-108 (sigmoid, xy=(s*2+grid)*stride, wh=(s*2)^2*anchor_grid, cat, view) for ONE level.
 * head: NHWC (bs,ny,nx, >= na*no) conv output; raw (may be NULL): contiguous (bs,na,ny,nx,no);
 * z (may be NULL): rows [row_offset, row_offset+na*ny*nx) of a contiguous (bs,total_rows,no) tensor.
 * anchors_px: na*2 floats on the HOST (anchor w,h in pixels = Detect.anchors[i]*stride[i]).
 * Arithmetic rounds after every op in `dtype`, as torch does for half tensors. */
int y3_detect_decode(const y3_tensor* head, int32_t dtype, int32_t na, int32_t no, const float* anchors_px,
                     float stride, void* raw, void* z, int64_t row_offset, int64_t total_rows, void* stream);
/* The same for n_levels (1..5) levels of one head in ONE launch of the tiled kernel of the 2-byte dtypes (16-byte loads and
 * stores, sigmoid from a 64 Ki-entry table of the very expression): heads[l], anchors_px[l*na*2 ..], strides[l],
 * raws[l] (raws or any entry may be NULL) and row_offsets[l] per level; z (may be NULL), total_rows, dtype, na, no common.
 * Every level must be eligible: f16 / bf16, 16-byte aligned head (pitch % 8 == 0), raw and z, and row_offset*no,
 * total_rows*no and ny*nx*no multiples of 8.  Otherwise (and with the knob decode_tile = 0) it returns non-zero, launches
 * NOTHING and sets y3_last_error: call y3_detect_decode per level, which takes the same kernel for eligible arguments and
 * the element kernels for the rest.  Results are bit for bit those of the per-level calls. */
int y3_detect_decode_levels(const y3_tensor* heads, int32_t n_levels, int32_t dtype, int32_t na, int32_t no,
                            const float* anchors_px, const float* strides, void* const* raws, void* z,
                            const int64_t* row_offsets, int64_t total_rows, void* stream);

/* Batched non_max_suppression: reference utils/general.py:630-750 incl. torchvision.ops.nms (:733).
 * pred: contiguous (bs, n_rows, 5+nc) of `dtype`.  Output: out_rows (bs, max_det, 6) fp32
 * [x1,y1,x2,y2,conf,cls] in descending-score order (score ties keep the reference's nonzero order, i.e.
 * torch.sort(stable=True)), out_counts (bs) int32.  classes: optional device int32 list.
 * Work space from y3_nms_workspace_bytes().  No host sync: counts stay on device. */
typedef struct {
    double iou_thres;           /* compared in double, as torchvision's CPU kernel does */
    float conf_thres;           /* rounded to `dtype` before the compares, as torch does for a python scalar */
    int32_t multi_label, agnostic;
    int32_t max_det, max_nms;   /* reference: 300 / 30000 */
    float max_wh;               /* reference: 7680 */
    int32_t n_classes_filter;   /* 0 = no class filter */
} y3_nms_params;
/* capacity = candidate slots for the whole batch; <= 0 picks the default (bs*16384, clamped to the
 * worst case bs*n_rows*nc).  Pass the same capacity to both calls. */
size_t y3_nms_workspace_bytes(int32_t bs, int32_t n_rows, int32_t nc, const y3_nms_params* p, int64_t capacity);
/* out_status (device, 2 x int32): [0] bit 0 = 1 if the candidate capacity overflowed (results invalid: call
 * again with a workspace sized for capacity >= out_status[1]), the bits above it = the number of images that took
 * the second round (knob nms_head; diagnostics); [1] = total candidates found. */
int y3_nms(const void* pred, int32_t dtype, int32_t bs, int32_t n_rows, int32_t nc, const y3_nms_params* p,
           const int32_t* classes, float* out_rows, int32_t* out_counts, int32_t* out_status, int64_t capacity,
           void* workspace, size_t workspace_bytes, void* stream);

/* Output edge after NMS, batched (csrc/val_edge.hip).
 * y3_scale_boxes: reference utils/general.py:613-626 scale_boxes + upstream clip_boxes (callers val.py:397,403, detect.py:223),
 * in place on fp32 xyxy rows: row r of image i starts at rows + i*img_stride + r*row_stride (floats; row_stride >= 4 so both the
 * (bs, max_det, 6) NMS output and an (n, 4) view work).  counts (DEVICE, may be NULL = max_rows rows per image); params: DEVICE
 * (bs, 5) fp32 {gain, pad_x, pad_y, w0, h0} computed by the caller exactly as the reference does (ratio_pad or the shapes).
 * y3_match_detections: reference val.py:147-188 process_batch with upstream box_iou, for every image: dets as above
 * ([x1,y1,x2,y2,conf,cls], row_stride >= 6), labels DEVICE (nl, 5) fp32 [cls,x1,y1,x2,y2] grouped by image through
 * label_offsets (DEVICE, bs+1 int32), iouv DEVICE (niou) fp32; correct: DEVICE (bs, max_det, niou) bytes (0/1), rows beyond
 * counts[i] are 0.  max_det <= 4096. */
/* Input edge: reference utils/augmentations.py:104-134 letterbox(auto=False) -- cv2.resize(INTER_LINEAR) to (new_h, new_w),
 * cv2.copyMakeBorder(color) to (H1, W1) -- fused with the HWC -> CHW transpose of models/common.py:867, one image per call.
 * src: DEVICE (h0, w0, cs) uint8, cs >= 3 interleaved channels (the first 3 are used); dst_batch: DEVICE (n, 3, H1, W1) uint8,
 * image `index` is written.  new_h/new_w/top/left are computed by the caller exactly as the reference does (Python round()). */
int y3_letterbox_u8(const uint8_t* src, int32_t h0, int32_t w0, int32_t cs, uint8_t* dst_batch, int32_t index, int32_t H1,
                    int32_t W1, int32_t new_h, int32_t new_w, int32_t top, int32_t left, int32_t color, void* stream);
/* Test-time augmentation edges: reference models/yolo.py:239-276 (_forward_augment, _descale_pred, _clip_augmented).
 * y3_scale_img: upstream ultralytics.utils.torch_utils.scale_img (un-vendored) fused with the `x.flip(3)` of models/yolo.py:246 -- NCHW (n, c, h, w)
 * -> NCHW (n, c, oh, ow): the (optionally left-right mirrored) batch resized like F.interpolate(size=(ih, iw), mode="bilinear",
 * align_corners=False), pad_value (the reference's 0.447) right / below up to (oh, ow).  The caller computes ih = int(h ratio), iw = int(w ratio),
 * oh = ceil(h ratio / gs) gs, ow likewise, as the reference does.  src != dst.
 * y3_descale_pred: rows [row0, row0 + nrows) of every image of a decoded prediction (bs, src_rows, no) -> rows [dst_row0, ...) of the concatenated
 * (bs, dst_rows, no) result, xywh / scale, flip 3: x = img_w - x, flip 2: y = img_h - y (0: none); every step rounded to dtype like the reference's
 * in-place tensor ops.  The row windows are _clip_augmented's. */
int y3_scale_img(const void* src, int32_t dtype, int32_t n, int32_t c, int32_t h, int32_t w, int32_t ih, int32_t iw, int32_t oh, int32_t ow,
                 int32_t flip_lr, float pad_value, void* dst, void* stream);
int y3_descale_pred(const void* src, int32_t dtype, int32_t bs, int32_t src_rows, int32_t no, int32_t row0, int32_t nrows, float scale,
                    int32_t flip, float img_h, float img_w, void* dst, int32_t dst_rows, int32_t dst_row0, void* stream);
/* The batch between the loader and model(imgs) in the reference's train loop (train.py:380, 394-399; utils/dataloaders.py:833-858), csrc/batch_edge.hip.
 * y3_resize_bilinear: NCHW (n, c, h, w) in Y3_U8 / Y3_F32 / Y3_F16 / Y3_BF16 -> NCHW (n, c, oh, ow) in Y3_F32 / Y3_F16 / Y3_BF16 (a uint8 output is unsupported):
 * F.interpolate(size=(oh, ow), mode="bilinear", align_corners=False) of to_f32(src) / divisor -- every tap divided (IEEE fp32) before the lerp, the
 * coordinate / weight arithmetic of y3_scale_img, one rounding to dst_dtype at the end.  divisor > 0; 255 with a uint8 source is `imgs.float() / 255` followed by
 * the --multi-scale resize, 1 leaves a floating batch as it is.  oh == h and ow == w give to_f32(src) / divisor exactly.  src != dst.
 * Stores are 16 bytes per lane when ow % 8 == 0 and dst is 16-byte aligned (every --multi-scale size is a multiple of 32); any other launch stores element by
 * element, with the same results.
 * y3_quad_collate_u8: collate_fn4 (--quad) on a uint8 batch (bs, c, h, w), bs % 4 == 0, -> uint8 (bs / 4, c, 2h, 2w) in one launch.  upsample_flags: bs / 4
 * bytes in device memory; group g with a non-zero flag is F.interpolate(im[4g].float(), scale_factor=2.0, mode="bilinear") truncated to uint8, the others are
 * images 4g / 4g+1 stacked top / bottom in the left half and 4g+2 / 4g+3 in the right half.  Bit-identical to torch.  src != dst. */
int y3_resize_bilinear(const void* src, int32_t src_dtype, int32_t n, int32_t c, int32_t h, int32_t w, void* dst, int32_t dst_dtype, int32_t oh,
                       int32_t ow, float divisor, void* stream);
int y3_quad_collate_u8(const uint8_t* src, int32_t bs, int32_t c, int32_t h, int32_t w, const uint8_t* upsample_flags, uint8_t* dst, void* stream);
int y3_scale_boxes(float* rows, int64_t img_stride, int32_t row_stride, const int32_t* counts, int32_t bs, int32_t max_rows,
                   const float* params, void* stream);
int y3_match_detections(const float* dets, int64_t img_stride, int32_t row_stride, const int32_t* counts, int32_t bs,
                        int32_t max_det, const float* labels, const int32_t* label_offsets, const float* iouv, int32_t niou,
                        uint8_t* correct, void* stream);

/* Statistics of a validation run, device-resident (csrc/val_stats.hip): reference val.py:386-428 after process_batch, utils/metrics.py:22-178.
 * Nothing here allocates or synchronises.  Rows of a run are three dense arrays: conf fp32, class int32, and the hits of the niou <= 16 IoU thresholds
 * as one bit mask (bit t = threshold t).
 * append: the valid rows of one batch (image i owns counts[i] rows, or max_det with counts == NULL) behind dst_offset, in image order.  conf / cls
 *   point at the first row's confidence / class; row r of image i lies at [i img_stride + r elem_stride] (the batched NMS output: rows + 4, rows + 5,
 *   6 max_det, 6; flat vectors: 0, 1 with bs = 1).  correct is the contiguous (bs, max_det, niou) result of the matching step.
 * count_labels: nt[class] += 1 for n label classes at cls[i stride] (classes outside [0, nc) are skipped).
 * compute: ap_per_class + compute_ap for the n rows held.  Order (class ascending, confidence descending, arrival ascending -- the last key is the
 *   documented tie rule), fp64 curves in the reference's operation order, then the summary.  conf_grid / recall_grid are DEVICE copies of
 *   np.linspace(0, 1, 1000) / np.linspace(0, 1, 101).  out (DEVICE doubles, at least out_elems(nc, niou)): out[0] classes with labels, out[1] the chosen
 *   confidence index, out[2] 1 if any row has a hit, out[3] the labels counted; then one row of niou + 6 per class with labels, ascending:
 *   [class, tp, fp, p, r, f1, ap[0 .. niou)].  workspace: 256-byte aligned, workspace_bytes(n, nc).
 * confusion_matrix: ConfusionMatrix.process_batch for a batch, one block per image, same inputs as the matching step (labels (nl, label_stride >= 5)
 *   [cls, x1, y1, x2, y2] grouped by image through label_offsets); adds into the DEVICE (nc + 1, nc + 1) int64 matrix[predicted][true].  Images without
 *   labels add nothing; dets == NULL with max_det 0 is the `detections=None` form (label_stride >= 1: classes alone).
 * labels_to_native: collate-format targets (nl, 6) [image, class, x, y, w, h] normalised, grouped by image -> (nl, 5) [class, x1, y1, x2, y2] in native
 *   pixels (val.py:371,401-403; params as scale_boxes: per image {gain, pad_x, pad_y, w0, h0}) and the bs + 1 label offsets. */
int y3_val_stats_append(const float* conf, const float* cls, int64_t img_stride, int32_t elem_stride, const int32_t* counts, int32_t bs,
                        int32_t max_det, const uint8_t* correct, int32_t niou, float* dst_conf, int32_t* dst_cls, uint16_t* dst_mask,
                        int64_t dst_offset, int64_t capacity, void* stream);
int y3_val_stats_count_labels(const float* cls, int32_t stride, int64_t n, int32_t* nt, int32_t nc, void* stream);
size_t y3_val_stats_out_elems(int32_t nc, int32_t niou);
size_t y3_val_stats_workspace_bytes(int64_t n, int32_t nc);
int y3_val_stats_compute(const float* conf, const int32_t* cls, const uint16_t* mask, int64_t n, const int32_t* nt, int32_t nc, int32_t niou,
                         double eps, const double* conf_grid, const double* recall_grid, double* out, size_t out_elems, void* workspace,
                         size_t workspace_bytes, void* stream);
int y3_confusion_matrix(const float* dets, int64_t img_stride, int32_t row_stride, const int32_t* counts, int32_t bs, int32_t max_det,
                        const float* labels, int32_t label_stride, const int32_t* label_offsets, int32_t nc, float conf_thres, float iou_thres,
                        int64_t* matrix, void* stream);
int y3_labels_to_native(const float* targets, int32_t nl, int32_t bs, float width, float height, const float* params, float* labels_out,
                        int32_t* offsets_out, void* stream);
/* The a-priori label rows of non_max_suppression(labels=...) / val.py --save-hybrid (utils/general.py:689-695, val.py:371-372), csrc/val_edge.hip: fills rows
 * [row0, row0 + n_rows) of every image of the (bs, total_rows, no) prediction `pred`.  targets: DEVICE (nl, 6) fp32 [image, class, x, y, w, h] grouped by image through
 * label_offsets (bs + 1 int32, as y3_labels_to_native writes them; the image column itself is not read).  Label k of image i -> row row0 + k:
 * xywh = targets[2:6] * (width, height, width, height) (fp32 product, rounded once to dtype), objectness 1, one-hot class 1, every other element 0; rows past the image's
 * labels are all 0, labels past n_rows are dropped.  A class outside [0, nc = no - 5) writes no one-hot (the reference raises IndexError): the row is never a candidate.
 * Rows outside the window are not touched.  Any `no` >= 6, any alignment. */
int y3_label_rows(const float* targets, int32_t nl, const int32_t* label_offsets, int32_t bs, float width, float height, void* pred, int32_t dtype,
                  int32_t total_rows, int32_t no, int32_t row0, int32_t n_rows, void* stream);
/* What a run writes (val.py --save-txt / --save-json, detect.py --save-txt, utils/plots.py:69-78 output_to_target), csrc/val_edge.hip: the per-box loops of val.py:98-103,
 * val.py:134-144 and detect.py:223-236 as ONE compact table for the batch.  rows / img_stride / row_stride / counts / bs / max_rows: the padded NMS result as y3_scale_boxes takes
 * it (row_stride >= 6; counts DEVICE, NULL = max_rows rows per image; views into a larger buffer work, elements past a row's sixth are not read).  Image i exports its first
 * n_i = min(counts[i], max_rows, limit) rows (limit 0: no cap; `o[:max_det]` of output_to_target): out (DEVICE, capacity rows of 7 fp32) rows [offsets[i], offsets[i + 1]), in
 * NMS order, or last to first with `reverse` (detect.py:231 `reversed(det)`); offsets (DEVICE, bs + 1 int32) is the exclusive prefix of n_i.  A row is
 *   Y3_EXPORT_TARGET  [image0 + i, cls, cx, cy, w, h, conf]                     cx = (x1 + x2) / 2, w = x2 - x1, pixels
 *   Y3_EXPORT_TXT     [image0 + i, cls, cx / w0, cy / h0, w / w0, h / h0, conf] sizes: DEVICE (bs, 2) fp32 native {w0, h0}, IEEE divisions
 *   Y3_EXPORT_JSON    [image0 + i, cls, cx - w / 2, cy - h / 2, w, h, conf]     the corner the reference computes, which is not bitwise x1
 * in fp32, operation for operation the reference's; `round_boxes` first rounds the four corners half to even (detect.py:223 `.round()`).  class_counts (DEVICE (bs, nc) int32, may be
 * NULL): class_counts[i][cls] += 1 for each of image i's n_i rows with cls in [0, nc) -- the export only adds: the CALLER zeroes it.  With counts given, rows that would land
 * at or past `capacity` are not stored (offsets[bs] and class_counts still hold the full count); with counts == NULL a capacity below bs * min(max_rows, limit) is an error.
 * One launch; nothing is read back.  -1 with y3_last_error set, before any launch, for null rows / offsets / out, bs <= 0, row_stride < 6, an unknown form, the txt form without
 * sizes, a histogram without classes and a capacity that is too small. */
enum { Y3_EXPORT_TARGET = 0, Y3_EXPORT_TXT = 1, Y3_EXPORT_JSON = 2 };
int y3_export_rows(const float* rows, int64_t img_stride, int32_t row_stride, const int32_t* counts, int32_t bs, int32_t max_rows, int32_t form, int32_t limit,
                   int32_t round_boxes, int32_t reverse, int32_t image0, const float* sizes, float* out, int64_t capacity, int32_t* offsets, int32_t* class_counts,
                   int32_t nc, void* stream);

/* Autoanchor, device-resident (csrc/autoanchor.hip): reference utils/autoanchor.py -- check_anchors.metric, anchor_fitness, print_results, the genetic loop
 * of kmean_anchors and the scipy.cluster.vq.kmeans call ahead of it.  Nothing here allocates or synchronises.  wh / pts are DEVICE (N, 2) fp32; k, f, v, codes,
 * dist and totals are DEVICE fp64 (8-byte aligned).  Limits: 1 <= n <= 64, 1 <= N < 2^31, R <= 64.  The per-point ratio metric x_j = min(min(r0, 1 / r0),
 * min(r1, 1 / r1)), r = wh / float(k_j), best = max_j x_j is fp32 with correctly rounded divisions; every sum is fp64 in a fixed order (bit-identical runs).
 * thr is the already inverted threshold 1 / anchor_t, compared in fp32 as torch compares a tensor with a Python scalar.
 * workspace_bytes: 8-byte aligned scratch of any of the three calls (R = 0: metrics / evolve alone); 0 and a message for a geometry out of range.
 * metrics: totals[0] sum of best over best > thr, [1] #(best > thr), [2] #(x > thr) over all N n, [3] sum x, [4] sum best, [5] sum of x over x > thr.
 * evolve: f = mean(best [best > thr]) of k, then for g in [0, gen): kg = max(k * v[g], 2.0) in fp64; if its fitness exceeds f (strict) k = kg, f = fg and
 *   accepted[g] = 1, else 0.  One launch per generation, stream-ordered, nothing read back; v is (gen, n, 2).
 * kmeans_step: one Lloyd iteration of R independent restarts (grid.y).  codes (R, n, 2) and live (R, n) int32 are read and rewritten: every point joins its
 *   nearest live code (Euclidean, ties to the lowest index), dist[r] = mean distance under the OLD codes (scipy.cluster.vq.vq), the codes become the means of
 *   their members, a live code without members goes dead for good (scipy's code_book[has_members]).  Restart r is skipped when bit r of `frozen` is set. */
size_t y3_anchor_workspace_bytes(int64_t N, int32_t n, int32_t R);
int y3_anchor_metrics(const float* wh, int64_t N, const double* k, int32_t n, float thr, double* totals, void* workspace, size_t workspace_bytes,
                      void* stream);
int y3_anchor_evolve(const float* wh, int64_t N, double* k, double* f, int32_t n, const double* v, int32_t gen, float thr, int32_t* accepted,
                     void* workspace, size_t workspace_bytes, void* stream);
int y3_kmeans_step(const float* pts, int64_t N, int32_t n, int32_t R, double* codes, int32_t* live, uint64_t frozen, double* dist, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Class and image weights of --image-weights training, device-resident (csrc/label_weights.hip): reference utils/general.py:543-568 labels_to_class_weights /
 * labels_to_image_weights and the random.choices call of train.py:363.  Nothing here allocates or synchronises.  cls is the DEVICE fp32 class column of every
 * label; a class id is the value truncated toward zero (astype(int)).  Limits: 1 <= nc <= 4096, 0 <= labels < 2^31, 1 <= images < 2^31.
 * label_histogram: counts is DEVICE int32 (nc + 1), overwritten: counts[c] = labels of class c at cls[i stride], counts[nc] = ids outside [0, nc) (NaN
 *   included) -- the error word (y3_val_stats_count_labels skips such ids silently and adds to what nt holds).  Integer atomics only: independent of order.
 * image_weights: offsets is DEVICE int64 (n_img + 1), image i owns the labels [offsets[i], offsets[i + 1]) (clamped to [0, n_labels]; empty allowed);
 *   iw[i] = sum over its labels of class_weights[id] (DEVICE fp64 (nc) / (n_img)), ids outside [0, nc) skipped.  One wave per image: lane l adds the labels
 *   first + l, first + l + 64, ... in ascending order, the 64 lane sums meet in an xor butterfly (32, 16, ..., 1) -- the order does not depend on the launch.
 * weighted_choices: random.choices(range(n), weights, k=k) for k uniforms u in [0, 1) drawn by the caller.  cum = inclusive fp64 prefix sum of weights (in the
 *   workspace; order: 8 consecutive weights per thread, Hillis-Steele over the 256 threads of a 2048-weight chunk, the same over the chunk totals -- fixed, so
 *   bit-identical run to run), total = cum[n - 1] + 0.0, out[j] = bisect_right(cum, u[j] total, 0, n - 1) for j < k, and the status word
 *   out[k] = 0, 1 (total <= 0: "Total of weights must be greater than zero") or 2 (total not finite).  out is DEVICE int64 (k + 1).
 * weighted_choices_workspace_bytes: 8-byte aligned scratch of weighted_choices (n cumulative weights + one carry per chunk); 0 and a message for n out of range. */
int y3_label_histogram(const float* cls, int32_t stride, int64_t n, int32_t* counts, int32_t nc, void* stream);
int y3_image_weights(const float* cls, int64_t n_labels, const int64_t* offsets, int64_t n_img, const double* class_weights, int32_t nc, double* iw, void* stream);
size_t y3_weighted_choices_workspace_bytes(int64_t n);
int y3_weighted_choices(const double* weights, int64_t n, const double* u, int64_t k, int64_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* COCO bbox evaluation of the run's COCO-JSON, device-resident (csrc/coco_eval.hip): pycocotools' COCOeval.computeIoU / evaluateImg / accumulate, which reference
 * val.py:464-477 runs on the host.  fp64 in pycocotools' operation order, integer counts: precision / recall / scores are its arrays bit for bit.  Nothing here
 * allocates or synchronises.  Limits: T <= 16, A <= 8, M <= 8, R <= 1024, detections and ground truths < 2^31, n_img * K < 2^31 - 1.
 * coco_match: det_img / det_cat DEVICE int64 (n_det) ids, det_box DEVICE fp64 (n_det, 4) [x, y, w, h], det_score fp64 (n_det); img_ids (n_img) / cat_ids (K) DEVICE
 *   int64, ascending and duplicate-free -- a detection whose image or category is in neither takes no part.  The ground truth is grouped by (image position,
 *   category position) in file order: gt_box fp64 (n_gt, 4), gt_area fp64 (the annotation's area), gt_crowd uint8, gt_cat int32 (category position), and
 *   gt_offsets DEVICE int32 (n_img * K + 1): pair p = image * K + category owns [gt_offsets[p], gt_offsets[p + 1]).  iou_thrs fp64 (T), area_rng fp64 (A, 2)
 *   inclusive bounds, max_det = the largest maxDets (only the first max_det detections of a pair, by score, are matched).
 *   Writes the rows in ACCUMULATE order (category position, score descending, image position, arrival): row_score fp64, row_rank int32 (rank inside the row's
 *   (image, category) pair; rows that take no part lie behind every category and keep what the buffer held), row_match / row_ignore uint16 (n_det, A), bit t =
 *   matched / ignored at threshold t; cat_begin / cat_end int32 (K): the rows of a category; npig int32 (K, A): ground truths not ignored (not crowd, area inside).
 * coco_accumulate: over the rows with rank < max_dets[m] of category k: tp / fp running counts of (match & ~ignore) / (~match & ~ignore), rc = tp / npig,
 *   pr = tp / (fp + tp + 2^-52) replaced by its reversed running maximum; recall[t, k, a, m] = last rc (0 without rows); for rec_thrs[r] the first j with
 *   rc[j] >= r gives precision[t, r, k, a, m] = pr[j] and scores[...] = score[j], 0 past the end.  Cells with npig == 0 are -1.  precision / scores DEVICE fp64
 *   (T, R, K, A, M), recall (T, K, A, M); max_dets DEVICE int32 (M), rec_thrs DEVICE fp64 (R).
 * coco_eval_workspace_bytes: 256-byte aligned scratch of coco_match; 0 and a message for arguments out of range. */
size_t y3_coco_eval_workspace_bytes(int64_t n_det, int64_t n_gt, int32_t T, int32_t A);
int y3_coco_match(const int64_t* det_img, const int64_t* det_cat, const double* det_box, const double* det_score, int64_t n_det, const int64_t* img_ids, int32_t n_img,
                  const int64_t* cat_ids, int32_t K, const double* gt_box, const double* gt_area, const uint8_t* gt_crowd, const int32_t* gt_cat, int64_t n_gt,
                  const int32_t* gt_offsets, const double* iou_thrs, int32_t T, const double* area_rng, int32_t A, int32_t max_det, double* row_score, int32_t* row_rank,
                  uint16_t* row_match, uint16_t* row_ignore, int32_t* cat_begin, int32_t* cat_end, int32_t* npig, void* workspace, size_t workspace_bytes, void* stream);
int y3_coco_accumulate(const double* row_score, const int32_t* row_rank, const uint16_t* row_match, const uint16_t* row_ignore, int64_t n_det, const int32_t* cat_begin,
                       const int32_t* cat_end, const int32_t* npig, int32_t K, int32_t T, const double* rec_thrs, int32_t R, const int32_t* max_dets, int32_t M, int32_t A,
                       double* precision, double* scores, double* recall, void* stream);

/* A cached dataset kept in device memory and batched without a host loader (csrc/dataset.hip): the augment=False path of reference utils/dataloaders.py:659-735
 * (LoadImagesAndLabels.__getitem__ over images cached already resized: the pad-only branch of letterbox, HWC -> CHW, BGR -> RGB, the two label conversions) and
 * collate_fn (:825-830).  Nothing here allocates or synchronises.
 * arena: DEVICE uint8, 16-byte aligned, arena_bytes a multiple of 4: every image (h, w, 3) BGR at images[i].offset.  images: DEVICE table of n_images records, 8-byte
 *   aligned; top / left are letterbox's round(dh - 0.1) / round(dw - 0.1) for the image's batch shape (bh, bw), computed by the host.  A batch is `count` images:
 *   indices[0 .. count) (DEVICE int64) or, with indices NULL, first .. first + count - 1.  An index outside [0, n_images), or a record that does not lie inside the
 *   arena or the batch width, yields an all-border image: no read leaves the arena.  Limits: W % 16 == 0, W <= 4096, H <= 65535, count * H < 2^25.
 * dataset_batch: dst is DEVICE (count, 3, H, W) of dst_dtype (Y3_U8 / Y3_F16 / Y3_BF16 / Y3_F32), contiguous, 16-byte aligned, written in one launch with 16-byte
 *   stores: element (b, c, y, x) = src_b[y - top_b][x - left_b][2 - c] inside the image, 114 outside; a floating output holds value / 255 (the fp32 IEEE quotient,
 *   rounded once to dst_dtype): what `im.to(dtype) / 255` gives.
 * dataset_targets: labels DEVICE fp32 (total, 5) [cls, x, y, w, h] normalised, label_offsets DEVICE int64 (n_images + 1).  Writes targets, DEVICE fp32 (n_rows, 6)
 *   [image in batch, cls, x, y, w, h] in image order, and offsets, DEVICE int64 (count + 1).  n_rows is the batch's label count, known to the caller from the
 *   offsets (rows past the device's own count are zeroed, rows past n_rows never written).  Per row, in fp32 and in the operation order of upstream xywhn2xyxy
 *   and xyxy2xywhn: x1 = w (xc - bw / 2) + padw, ... with padw = (W - w) / 2; clipped to [0, W - 1e-3] / [0, H - 1e-3] (the bounds formed in double and rounded to
 *   fp32 once); x = ((x1 + x2) / 2) / W, bw = (x2 - x1) / W.  count <= 1024. */
typedef struct {
    int64_t offset;         /* first byte of the image in the arena, a multiple of 16 */
    int32_t h, w;           /* the cached image */
    int32_t top, left;      /* rows / columns of border before it */
    int32_t bh, bw;         /* the batch shape top / left were computed for */
} y3_dataset_image;         /* 32 bytes */
int y3_dataset_batch(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const int64_t* indices, int64_t first, int32_t count,
                     void* dst, int32_t dst_dtype, int32_t H, int32_t W, void* stream);
int y3_dataset_targets(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const int64_t* indices, int64_t first,
                       int32_t count, int32_t H, int32_t W, float* targets, int64_t n_rows, int64_t* offsets, void* stream);

/* The same set kept in pinned HOST memory, one batch of it staged into a small device ring (csrc/dataset_stage.hip).  The host knows the images of a batch before any
 * pixel is touched, so dataset_stage copies just those, in ONE launch that reads the host arena over PCIe: the exports above and below then take (ring, dst_images)
 * where they take (arena, images) of a resident set.  Nothing here allocates or synchronises.
 * host_arena: HOST uint8, pinned and mapped (hipHostMalloc / hipHostRegister), 16-byte aligned, host_bytes a positive multiple of 16; its device-visible address is
 *   taken from hipPointerGetAttributes, and a range that is not pinned, mapped host memory is refused before anything is launched.  src_images: DEVICE table of
 *   n_images records whose `offset` is the image's first byte in host_arena, a multiple of 16.  dst_images: DEVICE table of n_images records, the ring's.
 * jobs: DEVICE int64 (m, 3), 8-byte aligned: per job the image, the offset of its slot in the ring (a multiple of 16) and the chunks of all jobs up to and including
 *   this one -- a job owns ceil(slot / y3_dataset_stage_chunk_bytes()) chunks, slot = 3 h w rounded up to 16; n_chunks is the last count, the launch's blocks.
 * Per job: ring[slot offset ..] = the image's 3 h w bytes, then zeros up to the slot's end, and dst_images[image] = src_images[image] with `offset` the slot's; no
 *   other record and no byte of the ring outside the slots is written.  Whatever the jobs and the records hold, no read leaves [host_arena, host_arena + host_bytes)
 *   and no write leaves the ring or dst_images: a job that would -- an image outside [0, n_images), a source range or a slot that does not fit, a misaligned offset,
 *   a chunk count above its predecessor's by another number than its slot's chunks -- is skipped by every block it owns, and its first block adds 1 to *status
 *   (DEVICE int32, which the caller zeroes once and reads when it reads the batch).  The table lives on the device, so what no block sees is the caller's to get
 *   right and is NOT reported: a job that owns no chunk (a running count equal to its predecessor's) is neither copied nor counted, and with n_chunks below the last
 *   running count the blocks past it do not run and the last jobs stay partly copied; dataset.stage_jobs (Python) forms the counts and n_chunks from one array.
 * Limits: m <= 8192 (m == 0 launches nothing), n_chunks < 2^31. */
int64_t y3_dataset_stage_chunk_bytes(void);
int y3_dataset_stage(const uint8_t* host_arena, int64_t host_bytes, const y3_dataset_image* src_images, int64_t n_images, const int64_t* jobs, int32_t m, int64_t n_chunks,
                     uint8_t* ring, int64_t ring_bytes, y3_dataset_image* dst_images, int32_t* status, void* stream);

/* The train-mode loader over the same arena and record table (csrc/augment.hip): the augment=True path of reference utils/dataloaders.py:659-735, 764-822
 * and utils/augmentations.py:57-73, 137-216, 270-283 -- mosaic, random_perspective (affine only), mixup, augment_hsv, the flips, collate_fn.  The host draws the random
 * numbers and sends one y3_augment_item per item of the batch (DEVICE, 8-byte aligned); nothing here allocates or synchronises.
 * A mosaic is a canvas of `canvas` x `canvas` pixels (2 S, or S for the letterbox branch) -- or, with canvas_h != 0, `canvas` wide and `canvas_h` high: the (W, H) of
 *   a rect=True batch, whose items take the letterbox branch -- filled with 114 on which tile t shows image `img`: canvas pixel (X, Y) of the
 *   rectangle [x1, x2) x [y1, y2) is image pixel (X - padw, Y - padh).  inv is the inverse of the affine matrix m (both row-major 2 x 3, float64).  An item blends
 *   two mosaics when nmos == 2: trunc(a * ratio + b * ratio1) in float64.  lut: the hue, saturation and value tables of augment_hsv, applied when hsv != 0.
 * augment_batch: dst is DEVICE (count, 3, S, S) of dst_dtype, contiguous, 16-byte aligned, written in one launch: per output pixel the flips undone, the source
 *   coordinate in 1 / 32 pixel ((rint((inv01 y + inv02) 1024) + 16 + rint(inv00 x 1024)) >> 5, likewise Y), four bilinear taps with integer weights (+ 512 >> 10),
 *   a tap outside the canvas or in no tile being 114; the blend; BGR -> HSV (integer, H in [0, 180)), the tables, HSV -> BGR (fp32); RGB planes; a floating output
 *   holds value / 255.  No read leaves the arena whatever the items and the records hold.  Limits: S % 16 == 0, 16 <= S <= 4096, count <= 1024.
 * augment_targets: every label row of the item's tiles, in tile order (the second mosaic's after the first's), through xywhn2xyxy(w, h, lpadw, lpadh) in fp32, the
 *   clip to [0, canvas] when clip != 0, the four corners through m in fp64, min / max, the clip to [0, S], box_candidates against the unwarped box times `scale`
 *   (wh_thr 2, ar_thr 100, area_thr 0.1, eps 1e-16), xyxy2xywhn(clip=True, eps=1e-3) and the flips.  Survivors are compacted in that order into targets, DEVICE
 *   fp32 (n_rows, 6) [item in batch, cls, x, y, w, h]; offsets, DEVICE int64 (count + 1), holds where every item's rows begin and, last, the survivor count.
 *   n_rows is the caller's upper bound (the label count of all tiles); rows past the survivor count are not written.
 * augment_polygons (a set with polygon labels; one launch ahead of the targets): vertices DEVICE fp32 (n_vertices, 2) normalised, vertex_offsets DEVICE int64
 *   (n_label_rows + 1): row r of the label table owns the vertices [vertex_offsets[r], vertex_offsets[r + 1]), an empty range meaning a row without a polygon; a range
 *   is clamped to [0, n_vertices].  Every label row of the tiles of every mosaic with clip != 0, at its position j in the order of augment_targets (item, mosaic, tile,
 *   row): per vertex x = w vx + lpadw, y = h vy + lpadh and the clip to [0, canvas] in fp32 (xyn2xy, np.clip); the polygon closed with vertex 0 and resampled to 1000
 *   points in fp64 as np.linspace(0, k, 1000) and np.interp give them (t_i = i (k / 999), t_999 = k; at t with q = floor(t): a = v_q where t == q, else
 *   (v_{q+1} - v_q) (t - q) + v_q); X = x m00 + y m01 + m02 and Y likewise, plain left-to-right fp64 sums; segment2box: over the points with 0 <= X <= S and
 *   0 <= Y <= S, boxes[j] = (min X, min Y, max X, max Y) and inside[j] = 1, or zeros and 0 when no point is kept or every kept X is zero.  paths, DEVICE int32
 *   (count, 2) per item and mosaic: bit 0 when some clipped coordinate of the mosaic's polygons is not zero, bit 1 when some label row of it has no polygon; 0 for a
 *   mosaic with clip == 0 or beyond nmos.  boxes DEVICE fp64 (n_rows, 4) and inside DEVICE int32 (n_rows), n_rows as for augment_targets; positions past n_rows are
 *   not written.  No read leaves the tables whatever the items and the offsets hold.
 * augment_targets_polygons: augment_targets, except that every row of a mosaic whose paths word is 1 (every row has a polygon, something is not zero) takes boxes[j]
 *   unclipped in place of the four warped corners and area_thr 0.01 in place of 0.1 (a row with inside[j] == 0 has a zero box and is dropped); every other mosaic runs
 *   the arithmetic of augment_targets.
 * augment_batch_hw / augment_targets_hw: the same two launches for items of H rows and W columns (the batch shape of a rect=True set): dst is (count, 3, H, W), the
 *   flips are W - 1 - x and H - 1 - y, the warped boxes are clipped to [0, W] x [0, H], then to [0, W - 1e-3] x [0, H - 1e-3] (formed in double, rounded to fp32
 *   once) and normalised per axis.  The reference's letterbox takes a rect batch's shape from a NumPy array, so its ratio and halves are float64 scalars and NumPy (>= 2)
 *   forms the product and the sum of xywhn2xyxy in float64: the tiles of such items carry wide != 0.  Limits: H % 16 == 0, W % 16 == 0, both in 16 .. 4096.  The square exports are these with H = W = S.  The polygon exports are
 *   square only. */
typedef struct {
    int32_t img;            /* index into the record table */
    int32_t x1, y1, x2, y2; /* the rectangle on the canvas */
    int32_t padw, padh;     /* canvas position of image pixel (0, 0) */
    float lpadw, lpadh;     /* the same for the labels (letterbox's halves may end in .5) */
    int32_t wide;           /* != 0: xywhn2xyxy forms w (x - bw / 2) + lpadw in float64 and rounds to fp32 once (a rect item, below); 0: fp32 throughout */
} y3_augment_tile;          /* 40 bytes */
typedef struct {
    double inv[6], m[6];
    double scale;           /* random_perspective's s */
    int32_t ntiles, canvas, clip;
    int32_t canvas_h;       /* the canvas height where it is not `canvas`; 0: a square canvas */
    y3_augment_tile tiles[4];
} y3_augment_mosaic;        /* 280 bytes */
typedef struct {
    y3_augment_mosaic mosaics[2];
    double ratio, ratio1;   /* mixup's r and 1 - r */
    int32_t nmos, flipud, fliplr, hsv;
    uint8_t lut[3][256];
} y3_augment_item;          /* 1360 bytes */
int y3_augment_batch(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, void* dst,
                     int32_t dst_dtype, int32_t S, void* stream);
int y3_augment_targets(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                       int32_t S, float* targets, int64_t n_rows, int64_t* offsets, void* stream);
int y3_augment_batch_hw(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, void* dst,
                        int32_t dst_dtype, int32_t H, int32_t W, void* stream);
int y3_augment_targets_hw(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                          int32_t H, int32_t W, float* targets, int64_t n_rows, int64_t* offsets, void* stream);
int y3_augment_polygons(const float* vertices, int64_t n_vertices, const int64_t* vertex_offsets, int64_t n_label_rows, const int64_t* label_offsets,
                        const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, double* boxes, int32_t* inside,
                        int32_t* paths, int64_t n_rows, void* stream);
int y3_augment_targets_polygons(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items,
                                int32_t count, int32_t S, const double* boxes, const int32_t* inside, const int32_t* paths, float* targets, int64_t n_rows,
                                int64_t* offsets, void* stream);

/* Copy-paste inside load_mosaic (csrc/augment.hip; reference utils/augmentations.py:219-240) for a set with polygon labels, launched only for a batch in which some
 * mosaic drew candidates; every other batch makes the launches above.  The host draws js = random.sample(range(n), k = round(p n)) per mosaic, n its polygons.
 * paste, DEVICE int32 (4 count + 1 + n_paste): 2 count + 1 offsets into js per (item, mosaic), then 2 count mask indices (-1: no paste), then the n_paste js of
 *   the batch.  A mosaic owns k positions directly after its tile rows in the position space of the polygon and targets launches: n_rows grows by n_paste.
 * copy_paste_select: one block per mosaic walks its js in order: label row j of labels4 (xywhn2xyxy and the clip of augment_targets) gives
 *   box = (2S - x2, y1, 2S - x1, y2) in fp32; it is accepted when ioa < 0.30 (fp32: the intersection, clip(0) per axis, over area(row) + 1e-7: bbox_ioa) against every
 *   row, rows appended by earlier candidates included.  sel_i DEVICE int32 (n_paste, 4): accepted, j, the label-table row of polygon j of the mosaic's list of
 *   polygons (not that of label row j in a mosaic that mixes polygon and box-only images), its tile; sel_f DEVICE fp32 (n_paste, 5): [cls, box].
 * copy_paste_raster: one block per accepted slot fills polygon j -- xyn2xy, the clip, the truncation of astype(int32) -- into masks, DEVICE int32 words
 *   (n_masks, 2S, 2S / 32) the caller has zeroed, bit x & 31 of word (y, x >> 5): drawContours(FILLED), 8-bit, shift 0, line_type 8, as
 *   tests/augment_copy_paste_cases.py::fill_mask restates it (8-connected boundary lines, scan-line spans (x_left + 65535) >> 16 .. x_right >> 16 over edges in 16.16).
 * batch_paste: augment_batch, except that a tap at canvas pixel (x, y) of a mosaic with a mask reads canvas pixel (2S - 1 - x, y) where bit (2S - 1 - x, y) is set.
 * polygons_paste / targets_paste: augment_polygons / augment_targets_polygons over the grown position space: an accepted slot carries the row [cls, box] and
 *   polygon j mirrored (fp32(2S) - x of the clipped vertex), an unaccepted slot is a dropped row; the path word is formed over the segments after the paste.
 * No read or write leaves the tables whatever the items, the offsets and the paste table hold.  Square items only; 2S % 32 == 0. */
int y3_augment_copy_paste_select(const float* labels, const int64_t* label_offsets, const int64_t* vertex_offsets, int64_t n_vertices, int64_t n_label_rows,
                                 const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, const int32_t* paste,
                                 int32_t n_paste, int32_t* sel_i, float* sel_f, void* stream);
int y3_augment_copy_paste_raster(const float* vertices, int64_t n_vertices, const int64_t* vertex_offsets, int64_t n_label_rows, const int64_t* label_offsets,
                                 const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, const int32_t* paste,
                                 int32_t n_paste, const int32_t* sel_i, int32_t* masks, int32_t n_masks, void* stream);
int y3_augment_batch_paste(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                           void* dst, int32_t dst_dtype, int32_t S, const int32_t* paste, const int32_t* masks, int32_t n_masks, void* stream);
int y3_augment_polygons_paste(const float* vertices, int64_t n_vertices, const int64_t* vertex_offsets, int64_t n_label_rows, const int64_t* label_offsets,
                              const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, const int32_t* paste,
                              int32_t n_paste, const int32_t* sel_i, const float* sel_f, double* boxes, int32_t* inside, int32_t* paths, int64_t n_rows, void* stream);
int y3_augment_targets_paste(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items,
                             int32_t count, int32_t S, const int32_t* paste, int32_t n_paste, const int32_t* sel_i, const float* sel_f, const double* boxes,
                             const int32_t* inside, const int32_t* paths, float* targets, int64_t n_rows, int64_t* offsets, void* stream);

/* The second-stage classifier hook of the detect loop (csrc/crops.hip): reference utils/general.py:827-859 apply_classifier (called at detect.py:202-203) for a whole
 * batch, and the box of upstream save_one_box (Detections.crop).  Nothing here allocates or synchronises.
 * rows / img_stride / row_stride / counts / bs / max_rows: the padded NMS result as y3_scale_boxes takes it, in the letterboxed space; rows are never written.
 * classifier_boxes: boxes DEVICE fp32 (bs, max_rows, 4), the reference's `d[:, :4]` after `.long()`: b = xyxy2xywh(row), with square != 0 w = h = max(w, h), w and h
 *   `* gain + pad` (a product, then a sum), xywh2xyxy, each coordinate truncated towards zero.  apply_classifier: gain 1.3, pad 30, square 1; save_one_box: 1.02, 10, 0.
 *   Rows at and beyond counts[i] are written as zeros and not read (counts NULL: every row is read).  One thread per detection.  y3_scale_boxes then runs on the table
 *   with row_stride 4: there is no second definition of that arithmetic.
 * crop_resize: arena / arena_bytes / images as for y3_dataset_batch (of a record only offset, h, w are read); image i of the batch is record i, n_images >= bs.
 *   boxes: the scaled, clipped table.  prefix: DEVICE int64 (bs), the exclusive prefix of the counts -- crop k of image i is tile prefix[i] + k of dst, DEVICE
 *   (n_tiles, 3, S, S) of dst_dtype (Y3_F16 / Y3_BF16 / Y3_F32), contiguous; n_tiles is the host's sum of the counts.  Per tile: the four coordinates truncated,
 *   h = y2 - y1, w = x2 - x1, cv2.resize(INTER_LINEAR) of the (h, w, 3) cutout to (S, S) in the 8-bit arithmetic of y3_letterbox_u8, every coordinate and coefficient
 *   relative to the cutout; plane c holds source channel 2 - c as value / 255 (the fp32 IEEE quotient, rounded once to dst_dtype).  16-byte stores when S % 8 == 0
 *   and dst is 16-byte aligned, element stores otherwise, the same values.  Whatever the tables hold, no read leaves an image's offset .. offset + 3 h w range or the
 *   arena and no write leaves dst: a tile whose cutout is empty (h < 1 or w < 1), whose box lies outside its image, whose image's record does not lie inside the
 *   arena or which the prefix and the counts do not place is written as zeros and adds 1 to *status (DEVICE int32, which the caller zeroes).  Limits: S in 1 .. 1024,
 *   n_tiles <= bs * max_rows, n_tiles * ceil(S / 16) < 2^31 (n_tiles == 0 launches nothing).
 * keep_matching: classes DEVICE int64 (n_tiles), the classifier's class per tile.  Writes out, DEVICE fp32 (bs, max_rows, 6) contiguous and distinct from rows: per
 *   image the rows whose (long) cls equals the class of their tile, in order, then zeros up to max_rows; and out_counts, DEVICE int32 (bs).  A tile crop_resize counts
 *   in *status never matches (the same test, on the same tables).  One block per image. */
int y3_classifier_boxes(const float* rows, int64_t img_stride, int32_t row_stride, const int32_t* counts, int32_t bs, int32_t max_rows, float gain, float pad,
                        int32_t square, float* boxes, void* stream);
int y3_crop_resize(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const float* boxes, const int32_t* counts,
                   const int64_t* prefix, int32_t bs, int32_t max_rows, void* dst, int32_t dst_dtype, int64_t n_tiles, int32_t S, int32_t* status, void* stream);
int y3_keep_matching(const float* rows, int64_t img_stride, int32_t row_stride, const int32_t* counts, const int64_t* prefix, int32_t bs, int32_t max_rows,
                     const int64_t* classes, int64_t n_tiles, const float* boxes, const y3_dataset_image* images, int64_t n_images, int64_t arena_bytes, float* out,
                     int32_t* out_counts, void* stream);

/* ComputeLoss: reference utils/loss.py:98-244 (build_targets :183-244, __call__ :131-181, criteria :104-129,
 * FocalLoss :31-63 when fl_gamma > 0) with upstream bbox_iou(CIoU) and smooth_bce.
 * preds: HOST array of nl DEVICE pointers, level i is contiguous (bs, na, ny[i], nx[i], nc+5) of `dtype`;
 * targets: DEVICE (nt, 6) fp32 [img, cls, x, y, w, h] normalised; anchors in grid units (Detect.anchors).
 * y3_loss_fwd writes out4 (DEVICE) = [ (lbox+lobj+lcls)*bs, lbox, lobj, lcls ] (gains applied, :176-181).
 * y3_loss_bwd (same params / preds / targets / workspace as the preceding fwd) overwrites grads[i] (same
 * shape and dtype as preds[i]) with d(out4[0]) / d preds[i] * grad_out[0] (grad_out: DEVICE scalar or NULL = 1).
 * Duplicate matches of one cell: tobj takes the LAST match in the reference's list order (CPU index_put), box/cls
 * gradients accumulate.  A target whose image index is outside [0, bs) or whose class is outside [0, nc) (the reference raises an
 * IndexError on the host) is skipped and turns out4 into NaN: the step fails loudly instead of reading out of bounds.  gr = 1 (the reference's value); autobalance: y3_loss_level_obj below. */
typedef struct {
    int32_t nl, na, nc, bs;
    int32_t ny[5], nx[5];
    float anchors[50]; /* [nl][na][2] */
    float balance[5];  /* reference: {4, 1, 0.4} for nl == 3, else first nl of {4, 1, .25, .06, .02}  (:122) */
    float anchor_t;    /* hyp['anchor_t'] */
    float box_gain, obj_gain, cls_gain; /* hyp['box'], hyp['obj'], hyp['cls'] (already scaled, train.py:327-329) */
    float cls_pw, obj_pw;               /* BCE pos_weight */
    float cp, cn;                       /* smooth_bce(label_smoothing) */
    float fl_gamma;                     /* 0 = plain BCE */
    int32_t sort_obj_iou;               /* ComputeLoss.sort_obj_iou (:101,156-158): a cell matched by several targets keeps its LARGEST iou as objectness target
                                           (the reference writes tobj in ascending-iou order); 0 = the last match in list order wins, the reference's default (ABI 3) */
} y3_loss_params;
size_t y3_loss_workspace_bytes(const y3_loss_params* p, int32_t nt);
int y3_loss_fwd(const y3_loss_params* p, int32_t dtype, const void* const* preds, const float* targets, int32_t nt,
                float* out4, void* workspace, size_t workspace_bytes, void* stream);
int y3_loss_bwd(const y3_loss_params* p, int32_t dtype, const void* const* preds, const float* targets, int32_t nt,
                const float* grad_out, void* const* grads, void* workspace, size_t workspace_bytes, void* stream);
/* ComputeLoss(autobalance=True), reference utils/loss.py:171-175: the per-level objectness losses `obji` of the forward that filled
 * `workspace` (same params / dtype / nt), nl device floats; the caller reads them back and moves its balance weights */
int y3_loss_level_obj(const y3_loss_params* p, int32_t dtype, int32_t nt, void* workspace, size_t workspace_bytes, float* obj_levels,
                      void* stream);

/* ---------------------------------------------------------------------------------------------- training
 * Train-mode `Conv` = act(bn(conv(x))) with BATCH statistics (reference models/common.py:75; BN eps 1e-3 / momentum
 * 0.03 set at models/yolo.py:229) and the autograd of the graph, decomposed as:
 *   forward : u = y3_conv2d_fwd(x)            (act NONE, zero bias; u is kept for the backward)
 *             y3_bn_stats(u) -> y3_bn_finalize (or y3_bn_stats_finalize) -> y = y3_bn_act_fwd(u [, residual])
 *   backward: du = y3_bn_act_bwd(u, dy)       (also gives dgamma, dbeta)
 *             dW = y3_conv2d_wgrad(x, du)     (fp32 OIHW, the layout of nn.Conv2d.weight.grad)
 *             dx (+)= y3_conv2d_fwd(du, filter packed by y3_pack_filter_dgrad [, residual = dx, in_dilation = stride])
 * `sums` is a caller-owned scratch of Y3_BN_SCRATCH_DOUBLES(C) doubles (totals + per-block partial rows; reductions
 * are atomics-free and deterministic); all per-channel vectors are DEVICE fp32. */
#define Y3_BN_SCRATCH_DOUBLES(C) ((size_t)(1 + 512) * 2 * (size_t)(C))
int y3_bn_stats(const y3_tensor* u, int32_t dtype, double* sums, void* stream);
int y3_bn_finalize(const double* sums, int64_t count, int32_t channels, const float* gamma, const float* beta, float eps,
                   float momentum, float* running_mean /* updated in place, may be NULL */, float* running_var,
                   float* scale, float* shift, float* mean, float* invstd, void* stream);
/* Training forward with the BatchNorm statistics taken in the conv epilogue (f16/bf16 MFMA path, no residual / upsample):
 * y3_conv2d_fwd plus, per (pixel tile, pixel wave) of the dispatched tile variant, one row [cout][2] fp32 of (sum, sum of
 * squares) of the STORED output values in stat_rows; *n_rows = rows written (query: y3_conv2d_fwd_stats_rows, -1 on error).
 * y3_bn_finalize_rows sums the rows in fp64 (fixed order; `sums` is a Y3_BN_SCRATCH_DOUBLES(C) scratch, totals land in its first
 * 2*C entries) and finalizes like y3_bn_finalize (count = n*h*w). */
int64_t y3_conv2d_fwd_stats_rows(const y3_conv_desc* desc, const y3_tensor* x, const y3_tensor* y);
int y3_conv2d_fwd_stats(const y3_conv_desc* desc, const y3_tensor* x, const void* packed_filter, const float* bias,
                        const y3_tensor* y, float* stat_rows, int64_t capacity_rows, int64_t* n_rows, void* stream);
/* the same with the scratch buffer of y3_conv2d_fwd_ws (the persistent kernel writes 4 rows per pixel tile: query with the same size) */
int64_t y3_conv2d_fwd_stats_rows_ws(const y3_conv_desc* desc, const y3_tensor* x, const y3_tensor* y, size_t workspace_bytes);
int y3_conv2d_fwd_stats_ws(const y3_conv_desc* desc, const y3_tensor* x, const void* packed_filter, const float* bias,
                           const y3_tensor* y, float* stat_rows, int64_t capacity_rows, int64_t* n_rows, void* workspace,
                           size_t workspace_bytes, void* stream);
int y3_bn_finalize_rows(const float* stat_rows, int64_t n_rows, int64_t count, int32_t channels, double* sums, const float* gamma,
                        const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* scale,
                        float* shift, float* mean, float* invstd, void* stream);
/* y3_bn_stats followed by y3_bn_finalize (count = n*h*w of u) with the partial-row sum and the finalize in one launch */
int y3_bn_stats_finalize(const y3_tensor* u, int32_t dtype, double* sums, const float* gamma, const float* beta, float eps,
                         float momentum, float* running_mean /* may be NULL */, float* running_var, float* scale, float* shift,
                         float* mean, float* invstd, void* stream);
int y3_bn_act_fwd(const y3_tensor* u, const float* scale, const float* shift, const y3_tensor* residual /* may be NULL */,
                  const y3_tensor* y, int32_t dtype, int32_t act, void* stream);
int y3_bn_act_bwd(const y3_tensor* u, const y3_tensor* dy, const float* scale, const float* shift, const float* mean,
                  const float* invstd, int32_t dtype, int32_t act, double* sums, const y3_tensor* du,
                  float* dgamma /* may be NULL */, float* dbeta /* may be NULL */, void* stream);
/* y3_bn_act_bwd for a unit with a residual input (`out = act(bn(conv(x))) + residual`, Bottleneck with shortcut): also writes
 * (gres_accumulate = 0) or accumulates (1) dy into the residual's gradient on the pass that reads dy anyway. */
int y3_bn_act_bwd_res(const y3_tensor* u, const y3_tensor* dy, const float* scale, const float* shift, const float* mean,
                      const float* invstd, int32_t dtype, int32_t act, double* sums, const y3_tensor* du, float* dgamma,
                      float* dbeta, const y3_tensor* gres, int32_t gres_accumulate, void* stream);
/* SyncBatchNorm (reference train.py:270-272 `--sync-bn`: torch.nn.SyncBatchNorm.convert_sync_batchnorm before DDP).  The host side all-reduces a few
 * fp64 words per layer between these calls (yolov3_amd/train_engine.py); everything stays on the device:
 *   forward : y3_bn_sum_rows (rows of a y3_conv2d_fwd_stats launch -> sums[0 .. 2C) = per-channel (sum, sum of squares); y3_bn_stats is the form that
 *             reads u) -> all-reduce(sums[0 .. 2C), element count) -> y3_bn_finalize_devcount (y3_bn_finalize with the count read from the device).
 *   backward: y3_bn_act_bwd_reduce (this rank's totals of (dz, dz xhat) in sums[0 .. 2C), dgamma / dbeta from them -- local, the gradient exchange
 *             averages them like every other parameter gradient -- and the local means in sums[2C .. 4C)) -> the host overwrites sums[2C .. 4C)
 *             with all-reduced totals / all-reduced count -> y3_bn_act_bwd_apply (du, and the residual's gradient as y3_bn_act_bwd_res).
 * y3_bn_act_bwd == reduce + apply back to back. */
int y3_bn_sum_rows(const float* stat_rows, int64_t n_rows, int32_t C, double* sums, void* stream);
int y3_bn_finalize_devcount(const double* sums, const double* count_dev, int32_t C, const float* gamma, const float* beta, float eps,
                            float momentum, float* running_mean, float* running_var, float* scale, float* shift, float* mean,
                            float* invstd, void* stream);
int y3_bn_act_bwd_reduce(const y3_tensor* u, const y3_tensor* dy, const float* scale, const float* shift, const float* mean,
                         const float* invstd, int32_t dtype, int32_t act, double* sums, float* dgamma /* may be NULL */,
                         float* dbeta /* may be NULL */, void* stream);
int y3_bn_act_bwd_apply(const y3_tensor* u, const y3_tensor* dy, const float* scale, const float* shift, const float* mean,
                        const float* invstd, int32_t dtype, int32_t act, const double* sums, const y3_tensor* du,
                        const y3_tensor* gres /* may be NULL */, int32_t gres_accumulate, void* stream);
/* Backward of the first layer (Conv(3, 32, 3, 1) + BatchNorm + act; no data gradient) in two passes over (u, dy) instead of three
 * plus a write: the reduction of y3_bn_act_bwd (totals into `sums`, dgamma, dbeta), then ONE kernel that applies the BatchNorm /
 * activation backward, rounds du to the storage dtype as y3_bn_act_bwd would have stored it, and accumulates
 * dw_oihw[32][cin][3][3] (fp32, the layout of nn.Conv2d.weight.grad) against the source image -- du never reaches memory.
 * x_nchw / src_dtype / divisor: the image exactly as y3_stem_conv_fwd received it.  32 filters, cin <= 3, f16 / bf16.
 * workspace: y3_stem_bn_bwd_wgrad_workspace_bytes() bytes (one fp32 partial tile per persistent block; summed in block order). */
size_t y3_stem_bn_bwd_wgrad_workspace_bytes(void);
int y3_stem_bn_bwd_wgrad(const void* x_nchw, int32_t src_dtype, int32_t n, int32_t cin, int32_t h, int32_t w, float divisor, const y3_tensor* u,
                         const y3_tensor* dy, const float* scale, const float* shift, const float* mean, const float* invstd, int32_t dtype,
                         int32_t act, double* sums, float* dgamma /* may be NULL */, float* dbeta /* may be NULL */, float* dw_oihw,
                         void* workspace, size_t workspace_bytes, void* stream);
/* OIHW fp32 -> filter bank of the data-gradient convolution: `cin` filters over (kh, kw, cout) with flipped taps. */
int y3_pack_filter_dgrad(const float* w_oihw, int32_t cout_src, int32_t cin_src, int32_t ksize, int32_t cout, int32_t cin,
                         int32_t dtype, void* packed, void* stream);
/* y3_pack_filter (forward bank) and y3_pack_filter_dgrad (data-gradient bank) of one layer in one launch (f16/bf16). */
int y3_pack_filter_pair(const float* w_oihw, int32_t cout_src, int32_t cin_src, int32_t ksize, int32_t cout, int32_t cin,
                        int32_t dtype, void* packed_fwd, void* packed_dgrad, void* stream);
/* y3_pack_filter_pair for MANY layers in one launch (the training step re-packs every layer's banks each step).  `jobs` is a DEVICE
 * array; job i occupies blocks [first_block, first_block + y3_pack_job_blocks(...)) of a grid of total_blocks 256-thread blocks, the
 * jobs laid out back to back in array order.  packed_fwd / packed_dgrad may be NULL (that bank is not wanted).  f16 / bf16.
 * Only the elements that come from a weight are written (source-indexed 32 x 32 tiles, round 5): ZERO-FILL a bank once when it is allocated -- its row / K
 * padding is never touched afterwards. */
typedef struct y3_pack_job {
    const float* w;          /* OIHW fp32 weights (nn.Conv2d.weight) */
    void* packed_fwd;        /* y3_packed_filter_elems(cout, cin, ksize) elements, or NULL */
    void* packed_dgrad;      /* y3_packed_filter_elems(cin, cout, ksize) elements, or NULL */
    int32_t cout_src, cin_src, ksize, cout, cin;
    int32_t first_block;
} y3_pack_job;
int64_t y3_pack_job_blocks(int32_t ksize, int32_t cout, int32_t cin, int32_t want_fwd, int32_t want_dgrad);
int y3_pack_filter_jobs(const y3_pack_job* jobs_device, int32_t n_jobs, int64_t total_blocks, int32_t dtype, void* stream);
/* Conv + BatchNorm fold AND pack of every layer of an inference plan in one launch (what yolov3_amd/engine.py did per layer with torch arithmetic and one
 * y3_pack_filter launch).  Per filter co: scale = gamma / sqrt(eps + var), w' = scale * w, b' = scale * b + (beta - gamma * mean / sqrt(var + eps)), b = conv_bias or 0,
 * evaluated in fp32 with IEEE sqrt / division and no FMA contraction (the operations of upstream fuse_conv_and_bn one by one: the results equal torch's bit for
 * bit), then w' is rounded to `dtype` (f16 / bf16 / f32) and written in the layout of y3_pack_filter -- or, stem != 0 (ksize 3, cin_src <= 4), of
 * y3_pack_filter_stem -- and b' to bias[0 .. cout_src).  A job without BatchNorm (the Detect heads) has the four bn_* pointers NULL: w' = w, b' = b.
 * `jobs` is a DEVICE array of 96-byte records; job i occupies blocks [first_block, first_block + y3_pack_job_blocks(ksize, cout, cin, 1, 0)) of the grid, the jobs
 * laid out back to back.  Only elements that come from a weight are written: ZERO-FILL banks and bias vectors once when they are allocated. */
typedef struct y3_fold_pack_job {
    const float* w;            /* OIHW fp32 weights (nn.Conv2d.weight) */
    const float* conv_bias;    /* cout_src floats, or NULL */
    const float* bn_gamma;     /* nn.BatchNorm2d weight / bias / running_mean / running_var, cout_src floats each; all four NULL: no BatchNorm */
    const float* bn_beta;
    const float* bn_mean;
    const float* bn_var;
    void* packed;              /* y3_packed_filter_elems(cout, cin, ksize) elements of `dtype` (stem: y3_packed_filter_stem_elems(cout)) */
    float* bias;               /* cout floats */
    float bn_eps;
    int32_t cout_src, cin_src, ksize, cout, cin;
    int32_t stem;
    int32_t first_block;
} y3_fold_pack_job;
int y3_fold_pack_jobs(const y3_fold_pack_job* jobs_device, int32_t n_jobs, int64_t total_blocks, int32_t dtype, void* stream);
/* Data gradient of a 3x3 stride-2 pad-1 conv without multiplying the zero taps of the dilated form: four output-parity
 * classes, each a small stride-1 conv of du (1, 2, 2 and 4 taps) with its own filter bank, written to every second
 * pixel of gx (+= residual when given; residual may alias gx).  f16/bf16 only. */
size_t y3_packed_filter_dgrad_s2_elems(int32_t cout, int32_t cin);
int y3_pack_filter_dgrad_s2(const float* w_oihw, int32_t cout_src, int32_t cin_src, int32_t cout, int32_t cin, int32_t dtype,
                            void* packed4, void* stream);
int y3_conv2d_dgrad_s2(int32_t dtype, const y3_tensor* du, const void* packed4, const y3_tensor* residual /* may be NULL */,
                       const y3_tensor* gx, void* stream);
/* filter gradient (and optional bias gradient = per-channel sum of du) of the conv described by `desc`
 * (dtype, ksize, stride, cin, cout = padded sizes of x / du); dw is (cout_real, cin_real, k, k) fp32, overwritten. */
size_t y3_conv2d_wgrad_workspace_bytes(const y3_conv_desc* desc, const y3_tensor* x);
/* dry run: the decision y3_conv2d_wgrad takes for (desc, x) WITH du->pitch == cout, real channel counts equal to the padded ones and no bias gradient --
 * tile edge (128 / 256; 0 = direct fp32 kernel), number of pixel slices (split-K over n*ho*wo) and whether a slice's tiles are grouped per XCD (knob
 * "wgrad_xcd"); tile 3 = the 3x3 strip kernel (csrc/wgrad_strip.h), slices = its persistent blocks; tile 4 = the padded-position kernel (csrc/wgrad_patch.h).
 * A launch with a bias gradient, real subsets or a wider du may take another form: y3_conv2d_wgrad_last_plan reports the one it took */
int y3_conv2d_wgrad_plan(const y3_conv_desc* desc, const y3_tensor* x, int32_t* tile, int64_t* slices, int32_t* xcd_grouped);
int y3_conv2d_wgrad(const y3_conv_desc* desc, const y3_tensor* x, const y3_tensor* du, int32_t cout_real, int32_t cin_real,
                    float* dw_oihw, float* dbias /* may be NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* the decision (as y3_conv2d_wgrad_plan reports one) of the last successful y3_conv2d_wgrad of this thread; fails before the first */
int y3_conv2d_wgrad_last_plan(int32_t* tile, int64_t* slices, int32_t* xcd_grouped);
/* backward of nn.Upsample(x2, nearest) / nn.MaxPool2d (+ZeroPad2d) / Detect's view+permute (models/yolo.py:98) */
int y3_upsample2x_bwd(const y3_tensor* dy, const y3_tensor* dx, int32_t dtype, int32_t accumulate, void* stream);
int y3_maxpool2d_bwd(const y3_tensor* x, const y3_tensor* dy, const y3_tensor* dx, int32_t dtype, int32_t k, int32_t stride,
                     int32_t pad, int32_t zpad_r, int32_t zpad_b, int32_t accumulate, void* stream);
/* The max-pool backward with a byte of workspace per OUTPUT element (y3_maxpool2d_bwd_workspace_bytes): pass 1 records each window's first maximum, pass 2 looks
 * the k^2 windows of an input element up -- k^2 byte loads per element where y3_maxpool2d_bwd scans k^2 windows of k^2 elements (SPP's 13 x 13 pool: 210 ms -> well
 * under a millisecond at batch 64).  Same sums in the same order.  Without a (large enough) workspace, or k > 15, it runs y3_maxpool2d_bwd. */
size_t y3_maxpool2d_bwd_workspace_bytes(const y3_tensor* x, int32_t k, int32_t stride, int32_t pad, int32_t zpad_r, int32_t zpad_b);
int y3_maxpool2d_bwd_ws(const y3_tensor* x, const y3_tensor* dy, const y3_tensor* dx, int32_t dtype, int32_t k, int32_t stride, int32_t pad, int32_t zpad_r,
                        int32_t zpad_b, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
int y3_detect_raw_bwd(const void* graw, int32_t dtype, int32_t bs, int32_t na, int32_t ny, int32_t nx, int32_t no,
                      const y3_tensor* ghead, void* stream);

/* Fused optimizer step: GradScaler.unscale_ + inf check, clip_grad_norm_(max_norm), SGD(nesterov)
 * with per-tensor lr / weight decay (reference utils/torch_utils.py:207-237: three parameter groups) and the ModelEMA
 * lerp (train.py:414-422), for ALL tensors in three launches.  `tensor_table`: DEVICE array of n_tensors records
 *   { float* param; const float* grad; float* momentum_buf; float* ema (or NULL); int64 numel; float lr, weight_decay;
 *     int32 first_chunk; int32 pad; }   (y3_sgd_tensor_record_bytes() == 56; chunks of 16384 elements)
 * scratch: n_chunks + 2 floats; scratch[0] = unclipped gradient norm, scratch[1] = clip coefficient after the call.
 * found_inf (device int32) = 1 when a gradient was inf/nan, in which case nothing is updated (GradScaler.step). */
size_t y3_sgd_tensor_record_bytes(void);
int y3_sgd_step(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, float max_norm, float momentum,
                int32_t nesterov, int32_t first_step, float ema_decay, float* scratch, int32_t* found_inf, void* stream);
/* The same step with the loss scale read from DEVICE memory (1 float), and torch.cuda.amp.GradScaler.update() (reference
 * train.py:345 `scaler = GradScaler(enabled=amp)`, :416-417 `scaler.step(optimizer); scaler.update()`; ATen _amp_update_scale_):
 * found_inf -> scale *= backoff_factor, tracker = 0; otherwise ++tracker and at growth_interval: scale *= growth_factor (if finite),
 * tracker = 0.  No host synchronisation anywhere. */
int y3_sgd_step_dynamic(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, const float* loss_scale, float max_norm,
                        float momentum, int32_t nesterov, int32_t first_step, float ema_decay, float* scratch, int32_t* found_inf,
                        void* stream);
int y3_loss_scale_update(float* loss_scale, int32_t* growth_tracker, const int32_t* found_inf, float growth_factor,
                         float backoff_factor, int32_t growth_interval, void* stream);
/* Fused Adam / AdamW / RMSProp steps: torch's single-tensor algorithms with fp32 state (amsgrad, maximize and centered off), behind the same two passes as
 * y3_sgd_step -- unscale + inf check + global norm + clip coefficient, then ONE streaming update that also does the ModelEMA lerp.  `tensor_table`: DEVICE array of
 *   { float* param; const float* grad; float* s1; float* s2; float* ema (or NULL); int64 numel; double lr, weight_decay, h0, h1, eps; int32 first_chunk; int32 pad; }
 * (y3_optim_tensor_record_bytes() == 96; chunks of 16384 elements).  Adam: s1 = exp_avg, s2 = exp_avg_sq, h0 / h1 = beta1 / beta2.  RMSProp: s1 = square_avg,
 * s2 = momentum buffer (NULL without momentum), h0 = alpha, h1 = momentum.  Pointers need 4-byte alignment; tensors whose pointers are all 16-byte aligned are streamed
 * 16 bytes at a time.  The gradients carry inv_scale^-1 (times *loss_scale when that DEVICE float is given; NULL: none).  `step`: DEVICE int32, the optimizer's step
 * count t; it advances (before the update, which reads it for the bias corrections) only when no gradient was inf/nan -- a skipped step changes nothing but
 * found_inf.  decoupled != 0: AdamW (p *= 1 - lr * wd, no decay in the gradient).  scratch / found_inf: as y3_sgd_step. */
size_t y3_optim_tensor_record_bytes(void);
int y3_adam_step(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, const float* loss_scale, float max_norm, int32_t decoupled,
                 float ema_decay, int32_t* step, float* scratch, int32_t* found_inf, void* stream);
int y3_rmsprop_step(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, const float* loss_scale, float max_norm, float ema_decay,
                    int32_t* step, float* scratch, int32_t* found_inf, void* stream);
/* ModelEMA.update(model) on its own (reference train.py:421): ema = d * ema + (1 - d) * src for every record of the DEVICE table, one launch, with the lerp
 * function of the fused steps above (the same bits as their ema pass).  Records of 32 bytes:
 *   { float* ema; const float* src; int64 numel; int32 first_chunk; int32 pad; }   (chunks of 16384 elements; n_chunks = their total)
 * 4-byte alignment is enough; tensors whose two pointers are 16-byte aligned are streamed 16 bytes at a time.  0 <= d <= 1. */
int y3_ema_update(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float d, void* stream);
/* The same lerp after a fused optimizer step, with ModelEMA's update count and decay kept on the DEVICE (added within ABI 6: nothing else changed).  `ema_state`:
 * 24 DEVICE bytes { int32 updates; float d; double decay; double tau; }.  Unless *found_inf is set (NULL: never), updates += 1 and d = decay * (1 - exp(-updates / tau)),
 * computed in double and rounded once, then every record is lerped with that d.  With *found_inf set -- the step before it was skipped -- nothing is written: the
 * averages stay bit for bit and the count does not advance, so the next update uses the decay of the updates really made.  No host synchronisation. */
int y3_ema_update_counted(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, void* ema_state, const int32_t* found_inf, void* stream);
/* The owner's step of the two-phase gradient exchange that replaces a bucket's all-reduce on a fully connected xGMI mesh (reference: DDP's gradient
   averaging, utils/torch_utils.py:60-72 smart_DDP / train.py:411): `parts` holds n_parts contributions of n floats each ([n_parts][n], what the all-to-all
   of the shards delivered); out[i] = (parts[0][i] + ... + parts[n_parts - 1][i]) * scale, added in that order.  `out` may alias none of `parts`. */
int y3_shard_mean(const float* parts, int32_t n_parts, int64_t n, float scale, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLOV3_HIP_H */
