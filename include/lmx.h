/* include/lmx.h -- C ABI of the MI355X-native LINEMOD template-matching engine (liblmx.so).
 *
 * Drop-in boundary.  Every entry point names the reference interface it replaces; paths are
 * relative to the reference repository (birlrobotics/linemod_pose_estimation):
 *
 *   lmx_match / lmx_match_batch   <-  cv::linemod::Detector::match(sources, threshold, matches, class_ids,
 *                                     noArray()) as called by rgbdDetector::linemod_detection,
 *                                     src/rgbdDetector.cpp:31-34 (decl include/linemod_pose_estimation/rgbdDetector.h:150);
 *                                     callers src/linemod_ensenso_detect_3_mult_detect_service.cpp:344,1190,
 *                                     src/linemod_ensenso_detect_3_mult_detect.cpp:321,1167, src/linemod_carmine_detect.cpp:348.
 *   lmx_bank_create / _add_class  <-  cv::linemod::Detector(modalities, T) + addTemplate results,
 *                                     src/renderer.cpp:179-185,308.
 *   lmx_bank_load_yaml            <-  readLinemod: Detector::read(fs.root()) + readClass per classes[] entry,
 *                                     src/rgbdDetector.cpp:1668-1680 (copies: src/renderer.cpp:42-54, ..._service.cpp:708-721).
 *   lmx_bank_save_yaml            <-  writeLinemod: Detector::write + writeClass, src/renderer.cpp:56-70.
 *   lmx_bank_num_classes/_class_id<-  Detector::classIds(), src/linemod_ensenso_detect_3_mult_detect.cpp:290.
 *   lmx_bank_get_template         <-  Detector::getTemplates(class_id, template_id),
 *                                     src/linemod_ensenso_detect_3_mult_detect_service.cpp:351.
 *   lmx_bank_num_templates, lmx_bank_T, lmx_bank_pyramid_levels <- Detector::numTemplates / getT / pyramidLevels.
 *
 * Plain C types only: pointers, sizes, fixed-width integers.  No C++/torch types cross this boundary.
 * All functions return lmx_status; lmx_last_error() gives the message of the calling thread's last failure.
 * Misuse that upstream signals with CV_Assert (source count != modality count, image size not a multiple
 * of T at some level, more than 63 features in a template) returns LMX_ERR_SHAPE; the C++ facade
 * (include/lmx_linemod.hpp) rethrows it as an exception like cv::Exception.
 *
 * There is NO CPU fallback: every compute entry point fails with LMX_ERR_NO_DEVICE when no gfx950 device
 * is usable.
 */
#ifndef LMX_H_
#define LMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum lmx_status {
  LMX_OK = 0,
  LMX_ERR_INVALID_ARG = 1,
  LMX_ERR_SHAPE = 2,      /* upstream CV_Assert equivalents */
  LMX_ERR_NO_DEVICE = 3,
  LMX_ERR_HIP = 4,
  LMX_ERR_OVERFLOW = 5,   /* candidate / match capacity exceeded; raise lmx_ctx_desc.max_candidates */
  LMX_ERR_IO = 6,
  LMX_ERR_PARSE = 7,
  LMX_ERR_NOT_FOUND = 8
} lmx_status;

enum { LMX_MOD_COLOR_GRADIENT = 0, LMX_MOD_DEPTH_NORMAL = 1 };

typedef struct lmx_bank lmx_bank; /* host-side template bank == the template state of cv::linemod::Detector */
typedef struct lmx_ctx lmx_ctx;   /* device context: a bank (or a shard of it) resident in HBM + per-frame workspaces */

/* Modality parameters (upstream defaults: ColorGradient(10, 63, 55), DepthNormal(2000, 50, 63, 2)). */
typedef struct lmx_modality_desc {
  int32_t type; /* LMX_MOD_* */
  float weak_threshold;
  float strong_threshold;
  int32_t num_features;
  int32_t distance_threshold;
  int32_t difference_threshold;
  int32_t extract_threshold;
} lmx_modality_desc;

typedef struct lmx_bank_desc {
  int32_t pyramid_levels;
  const int32_t* T; /* [pyramid_levels], e.g. {5, 8} (reference src/renderer.cpp:182-185) */
  int32_t n_modalities;
  const lmx_modality_desc* modalities;
} lmx_bank_desc;

/* A source image as the reference hands it to match(): possibly a strided ROI view
 * (src/linemod_ensenso_detect_3_mult_detect_service.cpp:324-326).  ColorGradient wants 8UC3 (channels 3,
 * elem_size 1), DepthNormal 16UC1 depth in mm (channels 1, elem_size 2). */
typedef struct lmx_image {
  const void* data;
  int32_t rows, cols;
  int32_t channels;
  int32_t elem_size;
  size_t row_stride_bytes;
} lmx_image;

/* cv::linemod::Match with class_id replaced by its index in lmx_bank_class_id() order (std::map order). */
typedef struct lmx_match_t {
  int32_t x, y;
  float similarity;
  int32_t template_id;
  int32_t class_index;
} lmx_match_t;

/* Unsorted shard-local match record (what ranks exchange in the multi-GPU all-gather):
 * `order_key` restores upstream insertion order (class slot, template_id, coarse raster index). */
typedef struct lmx_raw_match_t {
  int32_t x, y;
  float similarity;
  int32_t template_id;
  int32_t class_index;
  int32_t frame;
  uint64_t order_key;
} lmx_raw_match_t;

typedef struct lmx_ctx_desc {
  int32_t device;         /* HIP device ordinal */
  int32_t width, height;  /* frame size at pyramid level 0; must satisfy the T divisibility of every level */
  int32_t max_batch;      /* frames resident at once (>= 1) */
  int32_t max_candidates; /* per-frame capacity of coarse candidates and of matches; 0 = default (65536) */
  int32_t shard_rank;     /* this context holds templates [rank*N/world, (rank+1)*N/world) of every class */
  int32_t shard_world;    /* 0 or 1 = whole bank */
  void* stream;           /* hipStream_t to run on, or NULL to create a private one */
  int32_t flags;          /* LMX_CTX_* */
} lmx_ctx_desc;
/* Capture the per-batch kernel chain of enqueue() into a hipGraph (one per output slot, frame set, batch size and threshold) and
 * replay it: one launch instead of ~9.  The captured chain consists of kernel nodes only.  Ignored while per-kernel profiling is on. */
#define LMX_CTX_HIPGRAPH 1
/* Three device "lanes": lane 0 = the context's stream, the others = private streams with their own intermediate buffers.
 * Output slots alternate between the lanes and lmx_ctx_max_outstanding() = 6 lmx_ctx_enqueue calls may be outstanding instead
 * of two, so each stream always has its next batch queued and the kernels of one lane fill the tails of the others' (+17 %
 * throughput at 64 frames per batch on MI355X).  Results are unchanged.  Ordering: the private lanes start behind the most
 * recent upload; collect() returns results oldest first and waits on its own slot only; lmx_ctx_sync, uploads and debug reads
 * wait for every lane; lmx_ctx_export_raw is ordered on the context's stream behind the enqueue that produced the records.
 * May be combined with LMX_CTX_HIPGRAPH (one graph per output slot, frame set, batch size and threshold; the graphs of different
 * lanes replay concurrently: BASELINE config 5's per-GPU shape, tests/test_gpu_parity.py::test_config5_...). */
#define LMX_CTX_OVERLAP 2
/* Zero-copy input: sources that lie in pinned host memory (lmx_host_alloc, hipHostMalloc, hipHostRegister) are NOT staged by the
 * host; one kernel per modality pulls them over PCIe straight from the caller's buffers and lmx_ctx_upload / lmx_match* return
 * while that transfer is in flight: the caller keeps the pixels unchanged until lmx_ctx_upload_wait() or until a collect of an
 * enqueue that read them has returned.  Costs no host CPU time, moves 44 GB/s (the staged default: 54 GB/s with two or more
 * copy threads).  Without this flag every source, pinned or not, is copied before the call returns ("callee copies, never retains
 * pointers": the boundary's contract). */
#define LMX_CTX_ASYNC_INPUT 4
/* Gray colour sources: every ColorGradient source is 8UC1 (a MONO8 camera frame) instead of 8UC3, and the colour pyramid holds one
 * byte per pixel.  Quantisation runs over one plane; the results equal, bit for bit, those of the same image copied into B, G and R
 * on a context without the flag (upstream's strongest-channel rule picks channel 0 of three equal channels; blur, Sobel and pyrDown
 * work per channel).  A gray context refuses 8UC3 colour sources (LMX_ERR_SHAPE), and lmx_ctx_upload_raw takes only `mono` colour
 * sources (there is no colour-to-gray conversion); a context without the flag refuses 8UC1 colour sources as before.  Combines with
 * every other flag and passes through lmx_group_desc.flags to the members. */
#define LMX_CTX_GRAY 8

/* ---- bank ---------------------------------------------------------------------------------------------- */
lmx_status lmx_bank_create(const lmx_bank_desc* desc, lmx_bank** out);
/* templates: int32 [n_pyramids * L * M][5] = {width, height, pyramid_level, feat_begin, feat_count}, entry
 * l*M+m of pyramid p at row p*L*M + l*M + m; features: int32 [n_features_total][3] = {x, y, label}. */
lmx_status lmx_bank_add_class(lmx_bank* bank, const char* class_id, int32_t n_pyramids, const int32_t* templates,
                              const int32_t* features, int64_t n_features_total);
/* Trainer side, SURVEY.md 8f row 3: cv::linemod::Detector::addTemplate(sources, class_id, object_mask, &bounding_box)
 * (reference call sites src/renderer.cpp:308, src/renderer_only_image.cpp:266).  The per-pixel work (quantised orientations
 * with their magnitudes, quantised normals, the pyrDown chain) runs on the device with the same kernels match() uses; the
 * greedy scattered feature selection (extractTemplate / selectScatteredFeatures / cropTemplates) is sequential host code.
 * Sources as for match() (8UC3 / 16UC1 mm, any size from 16x16 up, odd widths and heights included: no T divisibility is
 * needed to train); object_mask 8UC1 or NULL.  Every modality's num_features must leave 1 .. 63 features at every pyramid level
 * (it is halved per level): LMX_ERR_SHAPE otherwise, here and in lmx_bank_train_mesh.
 * *template_id is the new id within the class, or -1 when some level has fewer candidates than num_features (upstream
 * returns -1 and adds nothing); bounding_box = {x, y, w, h} of cropTemplates. */
lmx_status lmx_bank_add_template(lmx_bank* bank, int32_t device, const lmx_image* sources, int32_t n_sources, const char* class_id,
                                 const lmx_image* object_mask, int32_t* template_id, int32_t bounding_box[4]);
/* DepthNormal's NORMAL_LUT: upstream quantises a unit normal with `NORMAL_LUT[v3][v2][v1]`, a constant
 * `uchar [20][20][20]` of one-hot labels that OpenCV ships as data (modules/.../normal_lut.i; used by the reference's trainers
 * and its carmine node through cv::linemod::DepthNormal, src/renderer.cpp:180-185, src/linemod_carmine_detect.cpp:802-840).
 * That file is not part of the reference repository, so the table is DATA on the bank here: the device kernels, the trainer
 * (lmx_bank_add_template) and the context all read the bank's table, indexed exactly like upstream (byte v3*400 + v2*20 + v1;
 * v1, v2, v3 may reach 20 and then run into the next row/plane as C's flat layout does; flat indices >= 8000, an out-of-bounds
 * read upstream, give "no label").  Entries must be 0 or one of 1, 2, 4, ..., 128.
 *   lmx_default_normal_lut     the documented default generator (azimuth octant of (nx, ny); NOT upstream's values)
 *   lmx_bank_set_normal_lut    install a table (NULL: explicitly choose the default generator)
 *   lmx_bank_load_normal_lut   the same from a file: 8000 raw bytes, or text holding 8000 integers such as OpenCV's normal_lut.i
 *   lmx_bank_normal_lut_origin LMX_LUT_*: where the bank's table came from
 * A bank read from a *_templates.yml that has a DepthNormal modality but neither the `lmx_normal_lut` marker that
 * lmx_bank_save_yaml writes nor a side-car table (`<yml>.normal_lut`, or the file named by the environment variable
 * LMX_NORMAL_LUT) was trained against a table this library cannot see: its origin is LMX_LUT_UNKNOWN and lmx_ctx_create
 * refuses it (LMX_ERR_INVALID_ARG) until one of the calls above states which table to match with. */
#define LMX_NORMAL_LUT_SIZE 8000
enum { LMX_LUT_DEFAULT = 0, LMX_LUT_USER = 1, LMX_LUT_SIDECAR = 2, LMX_LUT_UNKNOWN = 3 };
lmx_status lmx_default_normal_lut(uint8_t* out /* [LMX_NORMAL_LUT_SIZE] */);
lmx_status lmx_bank_set_normal_lut(lmx_bank* bank, const uint8_t* lut /* [LMX_NORMAL_LUT_SIZE] or NULL */);
lmx_status lmx_bank_get_normal_lut(const lmx_bank* bank, uint8_t* out /* [LMX_NORMAL_LUT_SIZE] */);
lmx_status lmx_bank_load_normal_lut(lmx_bank* bank, const char* path);
int32_t lmx_bank_normal_lut_origin(const lmx_bank* bank);
/* For readers that build a bank from a foreign yml themselves (the cv::FileNode facade): unless a table was installed with
 * set/load, take the one named by the environment variable LMX_NORMAL_LUT, else mark the bank LMX_LUT_UNKNOWN. */
lmx_status lmx_bank_require_normal_lut(lmx_bank* bank);
/* lmx_bank_save_yaml writes upstream's layout plus one extra top-level key OpenCV's reader ignores, `lmx_normal_lut: default`
 * or `lmx_normal_lut: sidecar`; in the second case the table goes to `<path>.normal_lut` (8000 raw bytes). */
lmx_status lmx_bank_load_yaml(const char* path, lmx_bank** out);
lmx_status lmx_bank_save_yaml(const lmx_bank* bank, const char* path);
void lmx_bank_destroy(lmx_bank* bank);
/* Deep copy (the copy is independent of `bank`; same templates, modalities, T and NORMAL_LUT). */
lmx_status lmx_bank_clone(const lmx_bank* bank, lmx_bank** out);
/* 64-bit content hash of everything that determines match() results: T, modality parameters, NORMAL_LUT, every class id,
 * template and feature.  Equal banks -> equal fingerprints; used as the key of the device-context cache below. */
uint64_t lmx_bank_fingerprint(const lmx_bank* bank);

/* The reference's service node rebuilds its detector on EVERY request: readLinemod(template yml) in the constructor
 * (src/linemod_ensenso_detect_3_mult_detect_service.cpp:1784-1786 -> :204-264 -> :224, :708-721) and never frees it.  Two caches
 * make that cheap behind an unchanged call pattern:
 *   lmx_bank_load_yaml_cached: process-wide cache keyed by (path, mtime, size), backed by a binary side file: the yml is parsed
 *     once, later calls (and later processes) get the same immutable bank (reference-counted; give it back with lmx_bank_release, never lmx_bank_destroy, never modify it).
 *   lmx_ctx_acquire / lmx_ctx_unref: process-wide cache of device contexts keyed by (bank fingerprint, every lmx_ctx_desc
 *     field): a detector built again from the same templates for the same frame size gets the context that is already
 *     resident in HBM instead of uploading the bank again.  The cached context owns a private copy of the bank, so the
 *     caller's bank may be modified or destroyed at any time.  lmx_ctx_unref only drops the reference; up to 8 idle contexts
 *     stay cached (least recently used goes first).  A context's calls must not overlap: see lmx_ctx_lock below (lmx_match / lmx_match_batch lock by themselves). */
lmx_status lmx_bank_load_yaml_cached(const char* path, const lmx_bank** out);
void lmx_bank_release(const lmx_bank* bank);
/* Compact binary form of a bank (templates, modalities, T, NORMAL_LUT; checksummed): a 3000-template RGB-D bank is 22.7 MB of
 * FileStorage YAML and 7 MB here, and loads in 14 ms instead of half a second (seconds with OpenCV's parser).
 * lmx_bank_load_yaml_cached keeps one next to the yml ("<yml>.lmxcache", tagged with the yml's mtime and size; written when the
 * directory allows it, LMX_NO_DISK_CACHE=1 disables), so a restarted node does not parse the YAML again either. */
lmx_status lmx_bank_save_binary(const lmx_bank* bank, const char* path);
lmx_status lmx_bank_load_binary(const char* path, lmx_bank** out);

/* The FileStorage-YAML document tree behind lmx_bank_load_yaml, for callers that walk a *_templates.yml themselves (the
 * cv::FileNode-shaped facade include/lmx_cv_linemod.hpp reads banks through Detector::read(FileNode) / readClass(FileNode)
 * like the reference's readLinemod, src/rgbdDetector.cpp:1668-1680).  Nodes are owned by the document. */
typedef struct lmx_yaml_doc lmx_yaml_doc;
typedef struct lmx_yaml_node lmx_yaml_node;
enum { LMX_YAML_NULL = 0, LMX_YAML_SCALAR = 1, LMX_YAML_SEQ = 2, LMX_YAML_MAP = 3 };
lmx_status lmx_yaml_open(const char* path, lmx_yaml_doc** out);
void lmx_yaml_close(lmx_yaml_doc* doc);
const lmx_yaml_node* lmx_yaml_root(const lmx_yaml_doc* doc);
int32_t lmx_yaml_kind(const lmx_yaml_node* node);
const char* lmx_yaml_scalar(const lmx_yaml_node* node);                       /* "" unless the node is a scalar */
int32_t lmx_yaml_size(const lmx_yaml_node* node);                             /* items of a sequence / entries of a map, else 0 */
const lmx_yaml_node* lmx_yaml_item(const lmx_yaml_node* node, int32_t i);     /* sequence item i / value of map entry i, or NULL */
const char* lmx_yaml_key(const lmx_yaml_node* node, int32_t i);               /* key of map entry i, or NULL */
const lmx_yaml_node* lmx_yaml_get(const lmx_yaml_node* node, const char* key); /* map lookup, or NULL */

int32_t lmx_bank_pyramid_levels(const lmx_bank* bank);
int32_t lmx_bank_T(const lmx_bank* bank, int32_t level);
int32_t lmx_bank_num_modalities(const lmx_bank* bank);
lmx_status lmx_bank_modality(const lmx_bank* bank, int32_t index, lmx_modality_desc* out);
int32_t lmx_bank_num_classes(const lmx_bank* bank);
const char* lmx_bank_class_id(const lmx_bank* bank, int32_t class_index); /* sorted (std::map) order */
int32_t lmx_bank_num_templates(const lmx_bank* bank, const char* class_id /* NULL = all classes */);
/* Template k = l*M+m of pyramid `template_id`; *features points at n_features x {x,y,label} owned by the bank. */
lmx_status lmx_bank_get_template(const lmx_bank* bank, const char* class_id, int32_t template_id, int32_t k,
                                 int32_t* width, int32_t* height, int32_t* pyramid_level, const int32_t** features,
                                 int32_t* n_features);

/* ---- device context ------------------------------------------------------------------------------------ */
lmx_status lmx_ctx_create(const lmx_bank* bank, const lmx_ctx_desc* desc, lmx_ctx** out);
void lmx_ctx_destroy(lmx_ctx* ctx);
/* Cached form (see lmx_bank_load_yaml_cached above).  *cache_hit (may be NULL) = 1 when an existing context was returned. */
lmx_status lmx_ctx_acquire(const lmx_bank* bank, const lmx_ctx_desc* desc, lmx_ctx** out, int32_t* cache_hit);
void lmx_ctx_unref(lmx_ctx* ctx);
/* Drops what the two process-wide caches hold without a user: device contexts nobody references (their device and pinned memory,
 * streams) and cached banks nobody references.  A long-running node with many template files may call it to give memory back; it also
 * matters for speed: an idle context alive in the process can cost ANOTHER context's pipelined matching 4-8 % (stream / hardware-queue
 * placement; scripts/idle_context_effect.py).  Referenced entries stay. */
void lmx_cache_trim(void);
/* A context's calls must not overlap.  The synchronous composites lmx_match / lmx_match_batch take the context's (recursive) lock
 * themselves, so callers that only use those -- e.g. two cv::linemod::Detector objects of the facade that were given the SAME cached
 * context by lmx_ctx_acquire, matching from two threads -- are serialised by the library.  Users of the split-phase calls
 * (upload / enqueue / collect / debug reads) that share a context across threads bracket their sequence with these. */
void lmx_ctx_lock(lmx_ctx* ctx);
void lmx_ctx_unlock(lmx_ctx* ctx);

/* "Next" row 4 of SURVEY.md 8f: the node-side steps immediately before match(), fused on the device so that the raw
 * camera frame is uploaded once and never touched by the host:
 *   MONO8 -> BGR by channel replication (mixChannels)          src/linemod_ensenso_detect_3_mult_detect_service.cpp:293-297
 *   cv::GaussianBlur(img, img, Size(3,3), 0, 0) on the FULL frame, then the crop Rect(bias_x, 0, 640, 480)   ...:324-326
 *   depth in float metres -> 16U millimetres, convertTo(CV_16UC1, 1000.0)   ...:837-858, src/linemod_carmine_detect.cpp:829-839
 * A source whose size equals (src_height, src_width) is cropped at (crop_x, crop_y) to the context's frame size; a source
 * that already has the context's size is taken as is.  Colour: 8UC3, or 8UC1 when `mono`; depth: 16UC1 mm, or 32FC1
 * metres when `depth_float_m`. */
typedef struct lmx_pre_desc {
  int32_t src_width, src_height;
  int32_t crop_x, crop_y;
  int32_t blur3;
  int32_t mono;
  int32_t depth_float_m;
} lmx_pre_desc;
lmx_status lmx_ctx_upload_raw(lmx_ctx* ctx, int32_t n_frames, const lmx_image* sources, int32_t n_sources, const lmx_pre_desc* pre);

/* Frames that already live in DEVICE memory (a decoder's, a simulator's, a torch tensor's, lmx_mesh_render's): lmx_image.data is a
 * device pointer on the context's device, row_stride_bytes any value >= the row's bytes; the address and the stride are multiples of the
 * element size (1, 2 or 4), nothing else is asked of alignment.  pre == NULL: frame-sized sources with the types lmx_ctx_upload takes,
 * copied as they are.  With `pre`: exactly lmx_ctx_upload_raw's meaning (crop of a src_width x src_height source, or a frame-sized one
 * taken as it is; 8UC3, or 8UC1 with `mono`; blur3 on the full frame; 16UC1 mm, or 32FC1 metres with depth_float_m), bit for bit.
 * No byte crosses PCIe and the host touches none: one ingest kernel per modality (k_ingest, timed as "k_pre") reads the images in
 * place and writes the next frame set's regular frame buffers, so enqueue, lmx_ctx_upload_masks (after this call), hipGraph contexts,
 * lanes and every collect form work as after lmx_ctx_upload.
 * Ordering (`stream` is the HIP stream that produces the frames; NULL = the null stream):
 *   - the sources are read AFTER everything queued on `stream` before the call: the library records an event there and its own ingest
 *     stream waits for it;
 *   - the call does NOT wait on the host for the ingest (the one host wait is the frame set's usual one, for the set's PREVIOUS upload);
 *   - before returning, `stream` is made to wait for the end of the ingest: work queued on `stream` afterwards may overwrite or free the
 *     sources (a torch tensor released to the caching allocator on that stream is safe).  Any other stream, or the host, calls
 *     lmx_ctx_upload_wait first: the end of the ingest is the set's transfer event.
 * Refused before anything is queued, the context stays usable: a pointer hipPointerGetAttributes does not report as plain device memory
 * of the context's device -- pageable, pinned, managed, another GPU's -- (LMX_ERR_INVALID_ARG, naming frame and source); an address or
 * stride that is no multiple of the element size (LMX_ERR_INVALID_ARG); a crop outside the source, wrong sizes or types (LMX_ERR_SHAPE,
 * as lmx_ctx_upload_raw); a `stream` that is being captured (LMX_ERR_INVALID_ARG); a context that is a member of a device group. */
lmx_status lmx_ctx_upload_device(lmx_ctx* ctx, int32_t n_frames, const lmx_image* sources, int32_t n_sources,
                                 const lmx_pre_desc* pre /* NULL: frame-sized sources taken as they are */, void* stream);

/* The drop-in call.  Clears nothing on the caller's side: writes up to `cap` matches in upstream output order
 * (std::sort + std::unique applied) and the total in *n_out (LMX_ERR_OVERFLOW if more than cap).
 * class_ids == NULL / n_class_ids == 0 matches every class (what the reference always passes). */
lmx_status lmx_match(lmx_ctx* ctx, const lmx_image* sources, int32_t n_sources, float threshold,
                     const char* const* class_ids, int32_t n_class_ids, lmx_match_t* out, size_t cap, size_t* n_out);
/* n_frames independent frames; sources[f*n_sources + m]; out[f*cap ...], n_out[f]. */
lmx_status lmx_match_batch(lmx_ctx* ctx, int32_t n_frames, const lmx_image* sources, int32_t n_sources, float threshold,
                           const char* const* class_ids, int32_t n_class_ids, lmx_match_t* out, size_t cap,
                           size_t* n_out);

/* Split-phase form of the same call, for inputs kept resident in HBM (bench, streaming, multi-GPU):
 *   upload  : host frames -> the NEXT of the context's frame sets (device frames + pinned staging each; one more set than
 *             device lanes), asynchronous on a private copy stream: the call copies pageable sources into the set's pinned
 *             staging with a few host threads (LMX_UPLOAD_THREADS, default min(8, cores/2)) and queues the transfer; it waits
 *             for no kernel.  The transfer of batch i+1 therefore overlaps the kernels of batch i, which is how the host-frame
 *             boundary of match() is pipelined: upload(i+1); enqueue(i+1); collect(i) ...
 *   enqueue : the whole kernel chain for frames [0, n_frames) of the most recently uploaded set, behind its transfer (device-
 *             side wait), no host synchronisation
 *   collect : wait for the OLDEST outstanding enqueue, take its match records (their read-back was queued behind its
 *             kernels), restore insertion order, std::sort + std::unique
 * Up to lmx_ctx_max_outstanding() enqueues may be outstanding (two output slots per device lane), so the host-side
 * finalisation of batch i overlaps the kernels of the following batches:  enqueue(0); loop { enqueue(i+1); collect(i); }
 * One enqueue more than that without a collect is an error. */
lmx_status lmx_ctx_upload(lmx_ctx* ctx, int32_t n_frames, const lmx_image* sources, int32_t n_sources);
/* Detector::match's last argument, `masks` (one 8UC1 Mat per modality, or an empty vector; the reference passes none,
 * src/rgbdDetector.cpp:33): the quantised labels of a modality survive where its mask is non-zero, at every pyramid level (upstream
 * QuantizedPyramid::quantize copies through the mask and halves the mask per level with INTER_NEAREST).  masks[f * n_masks + m] for the
 * first n_frames frames of the MOST RECENT upload (n_frames may be smaller than what was uploaded: the remaining frames are matched
 * unmasked); an entry with data == NULL means "no mask for this source".  The masks stay attached to those frames until the next upload
 * or the next lmx_ctx_upload_masks.  Batches with masks run the plain kernel chain (no graph replay, no fused small-batch launches). */
lmx_status lmx_ctx_upload_masks(lmx_ctx* ctx, int32_t n_frames, const lmx_image* masks, int32_t n_masks);
/* lmx_match with masks (masks == NULL: plain lmx_match): upload + upload_masks + enqueue + collect under the context's lock. */
lmx_status lmx_match_masked(lmx_ctx* ctx, const lmx_image* sources, const lmx_image* masks, int32_t n_sources, float threshold,
                            const char* const* class_ids, int32_t n_class_ids, lmx_match_t* out, size_t cap, size_t* n_out);
/* Host-side wait for the most recent upload's transfer (see LMX_CTX_ASYNC_INPUT). */
lmx_status lmx_ctx_upload_wait(lmx_ctx* ctx);
/* Pinned host memory for frames (camera drivers / benchmarks that want the zero-copy path): hipHostMalloc / hipHostFree. */
lmx_status lmx_host_alloc(size_t bytes, void** out);
void lmx_host_free(void* p);
/* Matches the first n_frames frames of the MOST RECENT upload (n_frames may be smaller than what was uploaded, not larger:
 * LMX_ERR_INVALID_ARG). */
lmx_status lmx_ctx_enqueue(lmx_ctx* ctx, int32_t n_frames, float threshold, const char* const* class_ids,
                           int32_t n_class_ids);
/* Per-class match thresholds.  What cv::linemod::Detector::match would produce if it passed thresholds[class] instead of `threshold` to
 * each matchClass call: classes are visited as for lmx_ctx_enqueue (the class_ids list when given, otherwise every class in the bank's
 * order), each with its own threshold in the coarse scan, the pruning bounds and the refinement, and one std::sort + std::unique runs over
 * everything.  thresholds[k] belongs to class index k (lmx_bank_class_id order) whether or not class_ids selects the class; n_thresholds
 * must equal the bank's class count; NaN is refused.  A bad argument returns LMX_ERR_INVALID_ARG and enqueues nothing.  With all entries
 * equal to t the result is lmx_ctx_enqueue's at t.  Enqueues with different thresholds may be outstanding together: the values travel in
 * a table per output slot, and with LMX_CTX_HIPGRAPH one captured chain serves every set of values. */
lmx_status lmx_ctx_enqueue_thresholds(lmx_ctx* ctx, int32_t n_frames, const float* thresholds, int32_t n_thresholds,
                                      const char* const* class_ids, int32_t n_class_ids);
/* lmx_match, lmx_match_batch and lmx_match_masked with per-class thresholds (see lmx_ctx_enqueue_thresholds). */
lmx_status lmx_match_thresholds(lmx_ctx* ctx, const lmx_image* sources, int32_t n_sources, const float* thresholds, int32_t n_thresholds,
                                const char* const* class_ids, int32_t n_class_ids, lmx_match_t* out, size_t cap, size_t* n_out);
lmx_status lmx_match_batch_thresholds(lmx_ctx* ctx, int32_t n_frames, const lmx_image* sources, int32_t n_sources, const float* thresholds,
                                      int32_t n_thresholds, const char* const* class_ids, int32_t n_class_ids, lmx_match_t* out, size_t cap,
                                      size_t* n_out);
lmx_status lmx_match_masked_thresholds(lmx_ctx* ctx, const lmx_image* sources, const lmx_image* masks, int32_t n_sources, const float* thresholds,
                                       int32_t n_thresholds, const char* const* class_ids, int32_t n_class_ids, lmx_match_t* out, size_t cap,
                                       size_t* n_out);
lmx_status lmx_ctx_collect(lmx_ctx* ctx, int32_t n_frames, lmx_match_t* out, size_t cap, size_t* n_out);
/* Same, frames packed back to back: frame f's matches are out[offsets[f] .. offsets[f+1]); offsets has n_frames+1 entries. */
lmx_status lmx_ctx_collect_flat(lmx_ctx* ctx, int32_t n_frames, lmx_match_t* out, size_t cap_total, size_t* offsets);

/* Multi-GPU plumbing: device pointers of the shard-local raw match records written by enqueue
 * (records: lmx_raw_match_t [capacity], all frames of the batch in one list, each tagged with its frame;
 * counts: uint32 [16] header, [0] = coarse candidates, [1] = records written) so a caller can all-gather
 * them over RCCL, and the host merge that turns gathered records of ONE frame into the final match list. */
lmx_status lmx_ctx_raw_matches(lmx_ctx* ctx, void** d_records, void** d_counts, size_t* capacity);
lmx_status lmx_merge_raw(const lmx_raw_match_t* records, size_t n_records, lmx_match_t* out, size_t cap, size_t* n_out);
/* Enqueue ONE device-to-device copy of this rank's gather block into a caller-owned device buffer (e.g. the send
 * buffer of an RCCL all-gather) on the context's stream.  Block layout (LMX_GATHER_HEADER_BYTES + capacity_records *
 * sizeof(lmx_raw_match_t) bytes): uint32 header[16] with header[0] = coarse candidates, header[1] = records written,
 * header[2] = capacity of the rank's candidate list (0 = not stated; header[0] > header[2] means candidates were dropped and
 * lmx_merge_gathered reports LMX_ERR_OVERFLOW), then the records.  Only the header and the first min(header[1], capacity_records) records are written; the rest of
 * the block keeps whatever it held. */
#define LMX_GATHER_HEADER_BYTES 64
lmx_status lmx_ctx_export_raw(lmx_ctx* ctx, void* d_block, size_t capacity_records);
/* The same copy on a caller-chosen stream (e.g. a communication stream that carries the all-gather): `stream` first waits,
 * on the device, for the most recent enqueue; nothing is queued on the context's own streams, so further enqueues are not
 * held up behind the exchange. */
lmx_status lmx_ctx_export_raw_on(lmx_ctx* ctx, void* d_block, size_t capacity_records, void* stream);
/* The same for the OLDEST outstanding enqueue (the one the next collect / release refers to) instead of the most recent one: a
 * pipelined caller that finds, when it finishes batch i, that its gather block was too small re-exports batch i's records --
 * they stay in the output slot until the slot is released -- into a larger block while later batches are already enqueued. */
lmx_status lmx_ctx_export_oldest_on(lmx_ctx* ctx, void* d_block, size_t capacity_records, void* stream);
/* The FINAL results of an enqueue left in device memory, for a next stage that also runs on the GPU: per frame the match list
 * Detector::match promises (insertion order restored, std::sort with libstdc++'s order of ties, std::unique) and, with `clusters`, the
 * clusters and members of lmx_ctx_collect_clusters -- bit for bit and in order what lmx_ctx_collect_flat / lmx_ctx_collect_clusters
 * return for the same enqueue, for every frame with status 0.  The counterpart of lmx_ctx_upload_device on the way out.
 * The call consumes nothing: the enqueue stays outstanding until lmx_ctx_collect* or lmx_ctx_release ends it, so a frame the export did
 * not finish can still go through the host path.
 * Outputs (plain device memory of the context's device; `lmx_cluster_t` 8-byte aligned, the others 4):
 *   header[16]        [0] n_frames, [1] flags, [2] total matches, [3] total clusters, [4] total members, [5] coarse candidates,
 *                     [6] raw records, rest 0.  Flags: 1 the slot's candidate or record list overflowed (nothing is delivered, every frame
 *                     has status 16, the totals are 0); 2 some frame was not finished (status 1 or 2); 4 some array did not fit.
 *                     The totals are the true ones, whatever fitted.
 *   frame_info[f][8]  {match_begin, match_count, cluster_begin, cluster_count, member_begin, member_count, status, raw_records}.
 *                     Frames lie back to back in frame order: a frame's *_begin is the sum of the counts of the frames before it whether
 *                     or not those fitted, and lmx_cluster_t.member_begin counts from the start of `members`, as lmx_ctx_collect_clusters
 *                     lays them out.  A frame's range of an array is written iff the WHOLE range fits that array's capacity (clusters
 *                     and members go together).  raw_records: the frame's records in the slot (0 with status 16).
 *                     status 0 delivered; 1 not finished: more than 2048 raw records and either none of this call's max_large_frames
 *                     left or more than 16384 records; 2 the chain's status 2 (a ring outside the packed range, `clusters` only); 4 / 8
 *                     or-ed onto 0: the frame's matches / its clusters or members did not fit; 16 list overflow.  Frames with status 1, 2
 *                     or 16 have counts 0 and add nothing to the offsets.
 * A capacity of 0 is allowed (nothing fits, the counts are still true).
 * Ordering (`stream` is the HIP stream that will consume the results; NULL = the null stream), lmx_ctx_upload_device's rules mirrored:
 *   - the export's kernels run on a private stream of the context, which waits ON THE DEVICE for the chosen enqueue and for what
 *     `stream` holds at the call (the outputs may still be in use there);
 *   - the call waits for nothing on the host and reads no result on the host: which frames need the large-frame kernel, the offsets
 *     and the fit tests are decided from device memory inside the kernels (the first call allocates the export's buffers, and a call
 *     with a larger max_large_frames than any before grows its workspace: 2.4 MB per frame);
 *   - before returning, `stream` is made to wait for the end of the export: work queued on `stream` afterwards may read the outputs.
 *     Any other stream, or the host, synchronises with `stream`;
 *   - lmx_ctx_release, every lmx_ctx_collect* form that ends the enqueue, lmx_ctx_sync and lmx_ctx_destroy wait (on the host) for the
 *     exports that read its slot before the slot can be reused.
 * Refused before anything is queued with LMX_ERR_INVALID_ARG, enqueue and context stay usable: a struct_size other than the struct's;
 * nothing outstanding; n_frames different from the enqueue's; a null header, frame_info or matches; `clusters` without a side-car
 * (lmx_ctx_set_cluster_sidecar) or with a null clusters_out or members; max_large_frames < 0; an output that hipPointerGetAttributes does
 * not report as plain device memory of the context's device, or that is not aligned to its element; a `stream` that is being captured; a
 * context that is a member of a device group. */
typedef struct lmx_export_desc {
  uint32_t struct_size;        /* sizeof(lmx_export_desc) */
  int32_t oldest;              /* 0: the most recent enqueue (as lmx_ctx_export_raw_on); 1: the oldest outstanding one (as lmx_ctx_export_oldest_on) */
  int32_t clusters;            /* 1: also voting .. NMS with the side-car of lmx_ctx_set_cluster_sidecar (mean similarity score) */
  int32_t max_large_frames;    /* frames of 2049 .. 16384 raw records this call may finish with the large-frame kernel; 0: none */
  uint32_t* header;            /* [16] */
  int32_t* frame_info;         /* [n_frames][8] */
  lmx_match_t* matches;
  size_t cap_matches;
  struct lmx_cluster_t* clusters_out;   /* clusters == 1 only */
  size_t cap_clusters;
  int32_t* members;            /* clusters == 1 only */
  size_t cap_members;
} lmx_export_desc;
lmx_status lmx_ctx_export_matches_on(lmx_ctx* ctx, int32_t n_frames, const lmx_export_desc* desc, void* stream);
/* The depth-scored, normal-scored and per-class clusters leave the same way: lmx_ctx_export_clusters_on, declared behind the types it
 * needs (lmx_depth_templates, lmx_depth_diff_t, lmx_normal_diff_t), after lmx_depth_templates_append. */
/* Copy `bytes` (multiple of 16, both pointers 16-byte aligned) on `stream` with a kernel instead of a DMA engine; `dst` may
 * be pinned host memory.  For small latency-sensitive read-backs in a pipelined caller: hipMemcpyAsync(DeviceToHost) was
 * measured to block the submitting thread for milliseconds now and then when copies of several streams are in flight. */
lmx_status lmx_stream_copy(void* dst, const void* src, size_t bytes, void* stream);
/* The same for `n_blocks` gather blocks (the result of an all-gather, one block per rank, `block_stride_bytes` apart in
 * both buffers): of every block only the header and the records it counts are copied, which is what lmx_merge_gathered
 * reads; a few KB over PCIe instead of n_blocks * capacity * 32 bytes. */
lmx_status lmx_stream_copy_blocks(void* dst, const void* src, int32_t n_blocks, size_t block_stride_bytes, size_t capacity_records, void* stream);
/* How many lmx_ctx_enqueue calls may be outstanding before one has to be collected (2; 6 with LMX_CTX_OVERLAP). */
int32_t lmx_ctx_max_outstanding(const lmx_ctx* ctx);
/* Drop the OLDEST outstanding enqueue without reading it back and free its output slot: waits (host) until it has
 * finished, like collect, but moves no data.  For callers that consume the records on the device (lmx_ctx_export_raw*). */
lmx_status lmx_ctx_release(lmx_ctx* ctx);
/* Host merge of `n_ranks` gathered blocks (each `block_stride_bytes` apart, layout above) into the final per-frame match
 * lists: frame f's matches are out[offsets[f] .. offsets[f+1]).  LMX_ERR_OVERFLOW if a rank wrote more records than
 * its block holds (raise the gather capacity) or cap_total is too small. */
lmx_status lmx_merge_gathered(const void* blocks, int32_t n_ranks, size_t block_stride_bytes, size_t capacity_records,
                              int32_t n_frames, lmx_match_t* out, size_t cap_total, size_t* offsets);
/* The same merge for a frame_groups x template_shards grid of ranks (see lmx_group below): n_ranks = G * R, rank k belongs to frame group
 * k / R and its records carry frame indices local to that group, whose frames are [g*n_frames/G, (g+1)*n_frames/G) of the batch.
 * frame_groups = 1 is lmx_merge_gathered. */
lmx_status lmx_merge_gathered_groups(const void* blocks, int32_t n_ranks, size_t block_stride_bytes, size_t capacity_records, int32_t n_frames,
                                     int32_t frame_groups, lmx_match_t* out, size_t cap_total, size_t* offsets);
/* ---- multi-GPU from the C++ side -------------------------------------------------------------------------
 * The caller of the hot path is C++ (rgbdDetector::linemod_detection, src/rgbdDetector.cpp:31-34): a group spreads a batch of frames
 * and the bank over several GPUs behind the same call shape.  The `world` members form a frame_groups x template_shards grid
 * (world = G * R, member k = frame group k / R, template shard k % R):
 *   member (g, r) pre-processes and matches frames [g*n/G, (g+1)*n/G) of a batch of n frames against templates [r*N/R, (r+1)*N/R)
 *   of every class.
 * G = 1 is pure template sharding (every member pre-processes the same frames: right for ONE frame's latency, BASELINE configs[3]);
 * R = 1 is pure frame sharding (every GPU holds the whole bank -- tens of MB at 50 000 templates -- and takes n/G of the frames: no
 * replicated pre-processing at all, right for streams of frames, BASELINE configs[4]).  Either way the only exchange is ONE RCCL
 * all-gather per batch of fixed-capacity per-member raw-record blocks (layout above), merged on the host exactly like the single-GPU
 * path (a member's records carry frame indices local to its group; lmx_merge_gathered_groups maps them back), so results are identical
 * for any G x R.  RCCL is dlopen'ed on first use.
 *   single process : n_devices GPUs (devices[] or 0..n-1), ncclCommInitAll; unique_id = NULL
 *   one process per GPU: unique_id = the 128 bytes lmx_group_unique_id produced on rank 0 (broadcast by the launcher), rank,
 *                    world, device
 * A rank that produces more records than gather_capacity does not fail: the exchanged headers carry the true counts, the blocks
 * are re-allocated to fit and the exchange is repeated (SURVEY 8e's two-phase fallback). */
typedef struct lmx_group lmx_group;
/* How the per-rank blocks are exchanged.  RCCL is the default and the only choice across processes.  PEER_COPY is a
 * single-process all-gather made of device-to-device block copies between the members' buffers (every member pulls the other
 * members' blocks on its own communication stream, ordered by events): no communicator, works between devices with peer access
 * AND between members that share a device, which RCCL refuses -- devices[] may then repeat a device id, so a group of any size
 * runs (and is tested) on a single GPU.  The environment variable LMX_GROUP_COLLECTIVE=rccl|peer overrides the field. */
#define LMX_GROUP_COLLECTIVE_RCCL 0
#define LMX_GROUP_COLLECTIVE_PEER_COPY 1
typedef struct lmx_group_desc {
  int32_t n_devices;         /* single-process mode */
  const int32_t* devices;    /* [n_devices] or NULL = 0..n_devices-1 */
  int32_t width, height, max_batch, max_candidates;
  int32_t gather_capacity;   /* records per rank in the all-gather block; 0 = 8192 */
  int32_t flags;             /* LMX_CTX_* for the member contexts */
  const void* unique_id;     /* multi-process mode: 128 bytes from lmx_group_unique_id, else NULL */
  int32_t rank, world, device;
  int32_t collective;        /* LMX_GROUP_COLLECTIVE_* */
  int32_t frame_groups;      /* G: 0 or 1 = template sharding only; must divide the number of members.  max_batch stays the size of the
                                whole batch the group accepts; a member's context holds ceil(max_batch / G) frames */
} lmx_group_desc;
lmx_status lmx_group_unique_id(void* out128);
lmx_status lmx_group_create(const lmx_bank* bank, const lmx_group_desc* desc, lmx_group** out);
void lmx_group_destroy(lmx_group* group);
int32_t lmx_group_size(const lmx_group* group);            /* members = frame_groups * template shards */
int32_t lmx_group_frame_groups(const lmx_group* group);   /* G */
int32_t lmx_group_gather_capacity(const lmx_group* group);   /* grows when a batch needed the two-phase fallback */
const char* lmx_group_collective_name(const lmx_group* group);   /* "rccl" or "peer_copy" */
/* lmx_match_batch over the group: out[f*cap ...], n_out[f], upstream output order.  = upload + submit + finish. */
lmx_status lmx_group_match_batch(lmx_group* group, int32_t n_frames, const lmx_image* sources, int32_t n_sources, float threshold,
                                 const char* const* class_ids, int32_t n_class_ids, lmx_match_t* out, size_t cap, size_t* n_out);
/* Split-phase form, mirroring lmx_ctx_upload / _enqueue / _collect (and linemod_pose_estimation_amd/dist.py ShardedMatcher):
 *   upload : the host frames are staged ONCE into pinned memory (one non-temporal copy by the group's host threads) and every
 *            member DMAs the same staging area into its own next frame set over its own PCIe link; waits for no kernel.
 *   submit : every member enqueues its kernel chain for the most recent upload and exports its records into the batch's send
 *            block on its communication stream (device-side wait on the enqueue); then ONE all-gather and the copy of rank 0's
 *            view (headers + counted records) into pinned host memory are queued.  Returns without waiting for the device; the
 *            members are driven by the group's host threads (one per member, at most 8).
 *   finish : waits for the OLDEST submitted batch, re-runs its exchange with larger blocks if a rank had more records than the
 *            block held (the records are still in the members' output slots), merges on the host, frees the members' slots.
 * Up to lmx_group_depth() batches may be in flight, so the exchange and the host merge of batch i overlap the kernels of the
 * following batches:  upload(0); submit(0); loop { upload(i+1); submit(i+1); finish(i); } */
lmx_status lmx_group_upload(lmx_group* group, int32_t n_frames, const lmx_image* sources, int32_t n_sources);
lmx_status lmx_group_submit(lmx_group* group, int32_t n_frames, float threshold, const char* const* class_ids, int32_t n_class_ids);
/* lmx_group_submit with per-class thresholds: every member forwards the same array to lmx_ctx_enqueue_thresholds. */
lmx_status lmx_group_submit_thresholds(lmx_group* group, int32_t n_frames, const float* thresholds, int32_t n_thresholds,
                                       const char* const* class_ids, int32_t n_class_ids);
lmx_status lmx_group_finish(lmx_group* group, int32_t n_frames, lmx_match_t* out, size_t cap, size_t* n_out);
int32_t lmx_group_depth(const lmx_group* group);

/* Synchronise the context's stream and fold pending profiling events (what collect does, without a read-back). */
lmx_status lmx_ctx_sync(lmx_ctx* ctx);

/* ---- "next" row 2 of SURVEY.md 8f: the immediate consumer of match() ------------------------------------------------
 * rcd_voting -> cluster_filter -> cluster_scoring (mean similarity) -> nonMaximaSuppressionUsingIOU, as chained by the nodes
 * (src/linemod_ensenso_detect_3_mult_detect_service.cpp:376-447; functions src/rgbdDetector.cpp:36-70, 72-85, 118-144, 462-574).
 * Host code on purpose: cluster membership depends on which duplicates std::unique removed, i.e. on libstdc++'s order of
 * ties in the final sort, so it must run on the finalised list.  Differences from the reference, both documented in
 * cluster_filter(map, thresh) erases while iterating (undefined behaviour there); here every cluster with
 * size <= thresh is removed.  `neighborSize` of the NMS is unused upstream (IoU threshold 0.4 is hard-coded). */
typedef struct lmx_cluster_params {
  int32_t vote_row_col_step;   /* clustering_step_ */
  double renderer_radius_min;
  double renderer_radius_step;
  int32_t cluster_size_thresh; /* clusters with size <= thresh are dropped (the nodes pass 2, carmine 0) */
} lmx_cluster_params;
typedef struct lmx_cluster_t {
  int32_t index[3];  /* {y / step, x / step, depth ring} */
  int32_t rect[4];   /* x, y, width, height: means over the cluster's matches (integer division) */
  double score;      /* mean similarity */
  int32_t member_begin, member_count; /* range in `members` (indices into `matches`, in cluster order) */
} lmx_cluster_t;
/* obj_origin_dists[template_id], rects[template_id][4] = {x, y, w, h} are the renderer-params side-car
 * (src/rgbdDetector.cpp:1681-1749).  Clusters come out in upstream's final order (sorted by score, NMS survivors only). */
lmx_status lmx_cluster_matches(const lmx_match_t* matches, size_t n_matches, const double* obj_origin_dists, const int32_t* rects,
                               size_t n_templates, const lmx_cluster_params* params, lmx_cluster_t* clusters, size_t cap_clusters,
                               size_t* n_clusters, int32_t* members, size_t cap_members);
/* As lmx_cluster_matches, but a cluster's score is the mean of match_values[i] over its members (in voting order) instead of the mean
 * similarity: with match_values[i] = (double)matches[i].similarity the two are equal bit for bit.  This is the slot of the reference's
 * second cluster score, getClusterScore over depth_normal_diff_calc (src/rgbdDetector.cpp:147-282, 576-584; commented out at both call
 * sites, :109-112 and :123-126, for its cost).  With the depth term alone that score is 1 / exp(mean depth difference in metres), exp is monotonic, so
 * match_values[i] = -(double)sum_abs_mm / (n_valid * 1000.0) of lmx_depth_diff_matches ranks the clusters in the same order; with the normal
 * term too, match_values[i] = lmx_match_value of lmx_normal_diff_matches' two results (the section on the normal term below).  A match
 * with n_valid == 0 has no such value; what it gets is the caller's choice (-HUGE_VAL sends every cluster that holds one to the end:
 * the Python helper's choice; leaving such matches out before the call is the other).  A cluster whose mean is NaN is refused
 * (LMX_ERR_INVALID_ARG): the score order would be undefined. */
lmx_status lmx_cluster_matches_scored(const lmx_match_t* matches, size_t n_matches, const double* match_values, const double* obj_origin_dists,
                                      const int32_t* rects, size_t n_templates, const lmx_cluster_params* params, lmx_cluster_t* clusters,
                                      size_t cap_clusters, size_t* n_clusters, int32_t* members, size_t cap_members);

/* ---- the chain for a bank of several classes --------------------------------------------------------------------------------------------
 * The reference runs one detector per object, each with its own `<object>_renderer_params.yml`
 * (src/linemod_ensenso_detect_3_mult_detect_service.cpp defines two such nodes).  With one bank of several classes the match list of a frame
 * holds every object's matches, and the chain above knows no classes: it would vote both objects into one bin, look template ids up in one
 * side-car and let the NMS suppress one object behind another.  lmx_cluster_matches_classes is the per-class composition:
 *   for each class c in ascending order with a side-car (classes[c].n_templates > 0):
 *     M_c = the matches with class_index == c, in the list's order;
 *     lmx_cluster_matches (match_values NULL) or lmx_cluster_matches_scored (on match_values of M_c) with classes[c];
 *     every member index mapped back to the match's position in `matches`;
 *   clusters = class 0's clusters in the chain's own order (score descending, NMS survivors only), then class 1's, ...;
 *   cluster_class[k] names cluster k's class.  The NMS never crosses classes.
 * Matches of a class without a side-car (n_templates == 0, or class_index >= n_classes) stay in `matches` and belong to no cluster; a
 * negative class_index is refused.  Every side-car's parameters are validated as by lmx_cluster_matches, also for a class without a match;
 * an error names the class.  LMX_ERR_OVERFLOW reports the full counts.
 * What this is NOT: the output of two single-class detectors.  Detector::match runs ONE std::sort + std::unique over all classes, here as
 * in cv::linemod, and std::unique removes only ADJACENT duplicates of (x, y, similarity, class): the other class's records sort in between
 * a class's duplicates, so which template of a duplicate survives, and whether both do, can differ from what a detector of object c alone
 * keeps.  Per class the set of (x, y, similarity) is the same; template ids, the number of matches, and hence the clusters' member
 * counts, scores and NMS survivors can differ.  Measured on two mesh-trained objects (profiles/two_object_chain.txt): the per-class
 * match lists equal the single-class detector's in 8 of 64 frames at threshold 85 and in none at threshold 80, the cluster lists in 48
 * and in none.  The composition above -- this function against lmx_cluster_matches per class on the SAME list -- is what holds exactly. */
typedef struct lmx_class_sidecar {
  const double* obj_origin_dists;   /* [n_templates] */
  const int32_t* rects;             /* [n_templates][4] */
  size_t n_templates;               /* 0: the class has no side-car */
  lmx_cluster_params params;
} lmx_class_sidecar;
lmx_status lmx_cluster_matches_classes(const lmx_match_t* matches, size_t n_matches, const double* match_values /* NULL: similarities */,
                                       const lmx_class_sidecar* classes, int32_t n_classes, lmx_cluster_t* clusters, int32_t* cluster_class,
                                       size_t cap_clusters, size_t* n_clusters, int32_t* members, size_t cap_members);

/* The renderer-params side-car that the consumer chain reads next to the matches: `<object>_renderer_params.yml`, written by the
 * reference's trainers (writeLinemodTemplateParams, src/renderer.cpp:72-130) and read by readLinemodTemplateParams
 * (src/rgbdDetector.cpp:1681-1749): per template "Template <i>": {R 3x3, T 3x1, K 3x3, D, Ori_dist, Rect}, then the renderer_* scalars.
 * obj_origin_dists / rects / renderer_radius_min / _step are exactly what lmx_cluster_matches and lmx_ctx_set_cluster_sidecar take
 * (Ori_dist and D pass through a float, as in the reference).  Arrays are owned by the struct: lmx_renderer_params_free. */
typedef struct lmx_renderer_params {
  size_t n_templates;
  double* obj_origin_dists;   /* [n] Ori_dist */
  int32_t* rects;             /* [n][4] Rect x, y, width, height */
  double* distances;          /* [n] D */
  double* R;                  /* [n][9] row major */
  double* T;                  /* [n][3] */
  double* K;                  /* [n][9] */
  int32_t renderer_n_points, renderer_angle_step, renderer_width, renderer_height;
  double renderer_radius_min, renderer_radius_max, renderer_radius_step;
  double renderer_focal_length_x, renderer_focal_length_y, renderer_near, renderer_far;
} lmx_renderer_params;
lmx_status lmx_renderer_params_load(const char* path, lmx_renderer_params** out);
lmx_status lmx_renderer_params_save(const lmx_renderer_params* params, const char* path);
void lmx_renderer_params_free(lmx_renderer_params* params);

/* The same consumer chain ON THE DEVICE, fed from the raw-match slot of an enqueue instead of a host list: one kernel per batch
 * (csrc/lmx_f2.hip, one workgroup per frame) restores upstream insertion order, applies Detector::match's std::sort + std::unique
 * and the reference's rcd_voting -> cluster_filter -> cluster_scoring -> nonMaximaSuppressionUsingIOU, reproducing libstdc++'s
 * order of ties in both sorts (csrc/lmx_sort_emul.hpp), so the output equals lmx_ctx_collect + lmx_cluster_matches for every
 * input.  Only the final matches and the surviving clusters cross PCIe.
 *   lmx_ctx_set_cluster_sidecar : obj_origin_dists[n_templates], rects[n_templates][4], parameters (copied to the device)
 *   lmx_ctx_collect_clusters    : replaces lmx_ctx_collect for the OLDEST outstanding enqueue.  Frame f's matches are
 *     matches[match_offsets[f] .. match_offsets[f+1]), its clusters clusters[cluster_offsets[f] .. cluster_offsets[f+1]);
 *     a cluster's members are members[member_begin .. member_begin + member_count), indices into ITS FRAME's matches.
 *     matches may be NULL (cap_matches 0) when only clusters are wanted.  Frames with more than 2048 raw records go to a second
 *     launch of the large-frame kernels (up to 16384 records; lmx_ctx_chain_stats); frames beyond that, or with a depth ring outside a
 *     kernel's packed range, are finished by the host path transparently.  The result is the same on every path. */
lmx_status lmx_ctx_set_cluster_sidecar(lmx_ctx* ctx, const double* obj_origin_dists, const int32_t* rects, size_t n_templates,
                                       const lmx_cluster_params* params);
lmx_status lmx_ctx_collect_clusters(lmx_ctx* ctx, int32_t n_frames, lmx_match_t* matches, size_t cap_matches, size_t* match_offsets,
                                    lmx_cluster_t* clusters, size_t cap_clusters, size_t* cluster_offsets, int32_t* members, size_t cap_members);

/* ---- training from a mesh: the reference's trainer (src/renderer.cpp:239-349, launch/start_object_renderer.launch) ----------------
 * The trainer renders the object's mesh from a list of view points, hands image + depth + silhouette to Detector::addTemplate and
 * writes `*_templates.yml` plus the `*_renderer_params.yml` side-car.  Here the renderer is a z-buffer rasteriser on the device
 * (csrc/lmx_mesh.hip; upstream's is OpenGL): per view (R, distance) the mesh is seen with X_cam = R X_obj + (0, 0, distance) through
 * the pinhole u = fx X / Z + cx, v = fy Y / Z + cy; a pixel is covered when its centre lies inside a triangle, the nearest triangle
 * wins (the lowest triangle index among equal depths), depth is perspective-correct, the shade of a face is Lambertian, two-sided,
 * 0.25 ambient: gray = rint(40 + 190 * (0.25 + 0.75 |n . l| / |n|)), depth_mm = rint(1000 z), both 0 off the object, mask 255 on it,
 * rect = {x, y, w, h} of the covered pixels ({0, 0, 0, 0} when none).  All of it in double, bit-identical on every run and batch size.
 * A view that puts a vertex at Z <= 0.01 is invalid: the call returns LMX_ERR_INVALID_ARG, the error text names the view's index,
 * and lmx_bank_train_mesh adds nothing to the bank.  The views themselves (upstream's RendererIterator) are the caller's input. */
typedef struct lmx_mesh_camera { int32_t width, height; double fx, fy, cx, cy; double light[3]; } lmx_mesh_camera;
typedef struct lmx_mesh_view   { double R[9]; double distance; } lmx_mesh_view;        /* X_cam = R X_obj + (0,0,distance) */
/* Renderer3d + RendererIterator::render as the trainers use them (src/renderer.cpp:239-275); outputs are host arrays, any may be NULL:
 * gray u8, depth_mm u16, mask u8 [n_views][height][width], rects int32 [n_views][4]. */
lmx_status lmx_mesh_render(int32_t device, const double* triangles /*[n][3][3] m*/, int32_t n_triangles, const lmx_mesh_camera* cam,
                           const lmx_mesh_view* views, int32_t n_views, uint8_t* gray, uint16_t* depth_mm, uint8_t* mask, int32_t* rects);
/* The trainer loop of src/renderer.cpp:262-329: render, addTemplate(sources, class_id, mask), keep the pose of every accepted view.
 * Views are rendered and quantised in batches on the device (the pixels never cross PCIe; the gray render feeds the one-plane colour
 * quantiser, whose templates equal those of the frame copied into B, G and R, so the result equals a loop of lmx_bank_add_template over
 * the rendered views: templates are appended in view order, a view addTemplate rejects adds nothing).  ColorGradient modalities get
 * the gray render, DepthNormal modalities the depth.  template_ids[v] = the new template id of view v, or -1.
 * *side_car (free with lmx_renderer_params_free) holds one entry per ACCEPTED view, filled as src/renderer.cpp:278-323 does:
 * Rect = silhouette rect, Ori_dist = the view's distance, R = the view's rotation, T = (0, 0, distance),
 * K = (fx, 0, width / 2; 0, fy, height / 2; 0, 0, 1) through float, D = Ori_dist - float(depth_mm[height / 2][width / 2]) / 1000.0f,
 * renderer_width / _height / _focal_length_* from the camera; the iterator's scalars (renderer_n_points, _angle_step, _radius_*,
 * _near, _far) start at 0 and are the caller's to set. */
lmx_status lmx_bank_train_mesh(lmx_bank* bank, int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam,
                               const lmx_mesh_view* views, int32_t n_views, const char* class_id,
                               int32_t* template_ids /*[n_views], -1 = rejected; may be NULL*/, lmx_renderer_params** side_car /*may be NULL*/);
/* The same trainer with options and statistics; opts == NULL is lmx_bank_train_mesh.  The bank, template ids, acceptance and side-car
 * are identical whatever the options say.
 * candidates = LMX_TRAIN_CANDIDATES_DEVICE: extractTemplate's per-pixel half (the mask erosions, DepthNormal's eight chessboard distance
 * transforms, the raster scan for candidates) runs on the device too, one workgroup per (view, pyramid level, modality) (csrc/
 * lmx_train_cand.hip), and only each window's candidate list crosses PCIe: 8-byte records in raster order {x | y << 14 | label << 28,
 * float score} behind a 64-byte header (count, area, label counts, status, offset; csrc/lmx_train_cand.hpp).  The host keeps the
 * division by the label counts, the stable sort, the scattered selection and cropTemplates.  Fallback rule: a view with a window (the
 * silhouette box grown by 2, per level) whose image, rows padded to 4 pixels, exceeds 65 536 bytes (every window of up to 40 000 pixels
 * fits, and square ones up to 256 x 256), or whose list does not fit the batch's record buffer, is rendered again after the regular
 * batches and trained through the packed read-back and the host's per-pixel code (n_fallback_views).
 * stats (may be NULL): n_device_views + n_fallback_views == n_views on the device path, both 0 on the host path; n_candidates and
 * list_bytes (headers + records) count the lists of the device views; the times are those of the LMX_MESH_TRAIN_TIMING line. */
#define LMX_TRAIN_CANDIDATES_HOST 0
#define LMX_TRAIN_CANDIDATES_DEVICE 1
typedef struct lmx_train_mesh_opts  { uint32_t struct_size; /* sizeof(lmx_train_mesh_opts) */ int32_t candidates; } lmx_train_mesh_opts;
typedef struct lmx_train_mesh_stats { int32_t n_views, n_accepted, n_device_views, n_fallback_views; int64_t n_candidates, list_bytes;
                                      double total_ms, device_wait_ms, host_select_ms; } lmx_train_mesh_stats;
lmx_status lmx_bank_train_mesh_opts(lmx_bank* bank, int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam,
                                    const lmx_mesh_view* views, int32_t n_views, const char* class_id, int32_t* template_ids,
                                    lmx_renderer_params** side_car, const lmx_train_mesh_opts* opts /*NULL = host*/,
                                    lmx_train_mesh_stats* stats /*may be NULL*/);
/* Test hook: the production candidate kernel on one caller-supplied window (the whole H x W image; mag == NULL: DepthNormal, mask ==
 * NULL: no object mask), then the production rank-and-select.  -> the list (records [n_records][2] words, label_counts[8], area) and
 * the selection (features [n_features][3], accepted).  LMX_ERR_SHAPE: the window is too large for the device path (the rule above) or
 * num_features is outside 1 .. 63; LMX_ERR_OVERFLOW: more than cap candidates. */
lmx_status lmx_debug_train_extract(int32_t device, const uint8_t* label, const float* mag, const uint8_t* mask, int32_t H, int32_t W,
                                   int32_t num_features, float strong_threshold, int32_t extract_threshold, uint32_t* records, size_t cap,
                                   size_t* n_records, uint32_t* label_counts, uint32_t* area, int32_t* features, int32_t* n_features,
                                   int32_t* accepted);

/* ---- depth check of matches against the rendered depth of their templates ------------------------------------------------------------
 * The depth half of the reference's depth_normal_diff_calc (src/rgbdDetector.cpp:147-282): lay the template's rendered depth over the
 * scene depth at the match position and average the absolute difference where both are valid.  Upstream re-renders the view per match;
 * a template's view never changes, so here the renders are made ONCE, cropped to their silhouette boxes and kept on the device
 * (lmx_depth_templates), and each match of a frame costs one pass over its crop (csrc/lmx_verify.hip, k_walk: one workgroup per
 * match).  Definition (csrc/lmx_depth_verify.hpp), for a crop t[h][w], a scene s[H][W] (both uint16 mm, 0 = not on the object / no
 * measurement) and a match at (x, y), any int32: crop pixel (i, j) meets scene pixel (x + j, y + i); it counts iff t != 0, the scene
 * pixel lies inside the image and s != 0.
 *   n_template = crop pixels with t != 0;  n_valid = counting pixels;  sum_abs_mm = sum of |t - s| over them.
 * Mean difference in mm = sum_abs_mm / n_valid; n_valid == 0 (nothing to compare, e.g. a crop entirely outside the image) is reported
 * as such.  Deviations from the reference: no vertical flip of the render, pixels outside the scene are skipped instead of
 * asserting, the difference is the signed one made absolute, and no 0 / 0.
 * The object owns a non-blocking stream and the buffers the scene frames, the match list and the results pass through (they grow on
 * demand); a mutex serialises calls on one object.  An object without any crop pixel touches no device until a call needs one. */
typedef struct lmx_depth_templates lmx_depth_templates;
typedef struct lmx_depth_diff_t { int64_t sum_abs_mm; int32_t n_valid; int32_t n_template; } lmx_depth_diff_t;
/* views[i] is template i's view (for a bank from lmx_bank_train_mesh: side_car->R[i], side_car->T[i][2]).  Renders on the device in
 * batches and keeps each view's silhouette box of the depth; a view that covers no pixel yields a 0 x 0 crop; a view with a vertex at
 * Z <= 0.01 fails the whole call (LMX_ERR_INVALID_ARG, the text names the view) before any device work. */
lmx_status lmx_depth_templates_from_mesh(int32_t device, const double* triangles, int32_t n_triangles, const lmx_mesh_camera* cam,
                                         const lmx_mesh_view* views, int32_t n_views, lmx_depth_templates** out);
/* ready-made crops (e.g. from the reference's own OpenGL trainer): crops[i] is [sizes[2i+1]][sizes[2i]] uint16, dense rows; sides
 * 0 .. 16384; a crop with a side of 0 is empty (kept as 0 x 0, its pointer is not read) */
lmx_status lmx_depth_templates_from_crops(int32_t device, const uint16_t* const* crops, const int32_t* sizes, int32_t n, lmx_depth_templates** out);
int32_t    lmx_depth_templates_count(const lmx_depth_templates* templates);
lmx_status lmx_depth_templates_rect(const lmx_depth_templates* templates, int32_t id, int32_t rect[4]);   /* from_mesh: silhouette box; from_crops: {0,0,w,h} */
lmx_status lmx_depth_templates_get(const lmx_depth_templates* templates, int32_t id, uint16_t* out /*[h][w]*/);  /* reads the crop back from the device */
/* bytes of device memory the templates occupy: the crops, rows padded to 16 bytes, and 24 bytes of table per template.  Not n x W x H.
 * The per-call buffers (scene frames, match list, results) are not counted. */
size_t     lmx_depth_templates_device_bytes(const lmx_depth_templates* templates);
void       lmx_depth_templates_free(lmx_depth_templates* templates);
/* depth[f]: 16-bit one-channel host images, all of one size, any row stride.  Frame f's matches are matches[offsets[f] .. offsets[f+1])
 * (offsets[0] == 0, non-decreasing).  class_index >= 0: matches of other classes get {0, 0, 0} and their template ids are not looked at.
 * out[i] belongs to matches[i].  A template_id outside [0, count) fails the call before any launch; the text names the match. */
lmx_status lmx_depth_diff_matches(lmx_depth_templates* templates, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                                  const size_t* offsets, int32_t class_index, lmx_depth_diff_t* out);
/* The value lmx_cluster_matches_scored and lmx_ctx_collect_clusters_depth average per cluster: minus the mean absolute difference in
 * metres, -((double)sum_abs_mm / ((double)n_valid * 1000.0)), or no_value when n_valid == 0 (and for a NULL diff).  One expression
 * (csrc/lmx_depth_verify.hpp, dv::value) for the device chain, the host fallback and every caller. */
double     lmx_depth_value(const lmx_depth_diff_t* diff, double no_value);

/* ---- depth-scored clusters on the device, straight from the raw-match slot ------------------------------------------------------------
 * lmx_ctx_collect_clusters ranks clusters by mean similarity; the composition lmx_ctx_collect + lmx_depth_diff_matches +
 * lmx_cluster_matches_scored ranks them by the depth difference but goes through the host's match list twice.  These two calls keep the
 * depth score on the device:
 *     lmx_ctx_enqueue(ctx, n, threshold, ...);
 *     lmx_depth_templates_upload_scene(templates, depth, n);            // returns at once: the transfer overlaps the match kernels
 *     lmx_ctx_collect_clusters_depth(ctx, n, templates, -1, -HUGE_VAL, ...);
 * upload_scene: depth[f] as lmx_depth_diff_matches takes them (16-bit, one channel, one size, any row stride).  The frames are staged into
 * the object's pinned buffer, their copies are queued on the object's stream and an event is recorded behind them; there is NO host
 * synchronisation.  The object remembers the scene (frame count, width, height) until the next upload_scene replaces it, which first waits
 * for the previous copies to leave the staging buffer; lmx_depth_diff_matches uses the same buffers and FORGETS the uploaded scene whenever it stages
 * frames of its own, that is whenever it has a match to check (a call without one returns early and leaves the scene): after any call of
 * it, upload the scene again.
 * collect_clusters_depth: lmx_ctx_collect_clusters for the oldest outstanding enqueue (same outputs, same context locking) with
 *   diffs[i]          = the depth check of matches[i] against scene frame f (parallel to matches; may be NULL; written when matches is),
 *   clusters[k].score = the mean over the cluster's members, in voting order, of lmx_depth_value(diffs[i], no_value).
 * On the context's consumer stream: wait for the scene's event, the record form of k_walk (one workgroup per RAW record: which of two duplicate
 * records std::unique keeps is decided by the sort that follows), the scored form of k_f2_finalize_cluster, one synchronisation.  Frames
 * of 2049 .. 16384 records are finished by the scored large-frame kernel from the same per-record results (lmx_ctx_chain_stats); frames
 * the device chain hands back (more than 16384 records, a ring outside the packed range) are finished on the host inside the call
 * (the job form of k_walk on the resident scene + lmx_cluster_matches_scored), with the errors lmx_ctx_collect_clusters reports for them.
 * For EVERY input matches, diffs, clusters (score included) and members equal, bit for bit,
 *     lmx_ctx_collect;  lmx_depth_diff_matches(templates, depth, n, matches, offsets, class_index, diffs);
 *     per frame lmx_cluster_matches_scored with match_values[i] = lmx_depth_value(&diffs[i], no_value)
 * -- that composition stays the one to use for values the caller computes himself (a learned score) and for matches he filtered before
 * clustering; the normal term of depth_normal_diff_calc has entry points of its own: lmx_normal_diff_matches and
 * lmx_ctx_collect_clusters_depth_normal below.  class_index >= 0: matches of other classes get zero diffs, hence no_value.
 * no_value: -HUGE_VAL sends every cluster that holds a match with nothing to compare to the end (the Python helper depth_values' choice).
 * LMX_ERR_INVALID_ARG, the enqueue staying outstanding, when: no side-car is set; templates lives on another device; no scene is uploaded,
 * or its frame count / width / height differ from the enqueue's frame count / the context's frame size; lmx_depth_templates_count differs
 * from the side-car's n_templates; no_value is NaN.  The object's mutex is held for the whole call. */
lmx_status lmx_depth_templates_upload_scene(lmx_depth_templates* templates, const lmx_image* depth, int32_t n_frames);
/* upload_scene for depth frames in DEVICE memory on the object's device (16UC1, one size, any even row stride): pitch-aware
 * device-to-device copies on the object's stream, no staging and no host wait, so the depth- and normal-scored chains run without a host
 * frame.  Ordering as lmx_ctx_upload_device: the frames are read after everything queued on `stream` (NULL = the null stream) before the
 * call; before returning, `stream` is made to wait for the copies, so work queued there afterwards may overwrite or free the frames; any
 * other stream, or the host, first waits for a scored collect (which runs behind the copies).  The same refusals, before anything is
 * queued: not plain device memory of the object's device, an odd address or stride, a capturing stream (LMX_ERR_INVALID_ARG); wrong
 * types or sizes (LMX_ERR_SHAPE).  The scene is remembered and forgotten exactly as upload_scene's. */
lmx_status lmx_depth_templates_upload_scene_device(lmx_depth_templates* templates, const lmx_image* depth, int32_t n_frames, void* stream);
lmx_status lmx_ctx_collect_clusters_depth(lmx_ctx* ctx, int32_t n_frames, lmx_depth_templates* templates, int32_t class_index, double no_value,
                                          lmx_match_t* matches, size_t cap_matches, size_t* match_offsets,
                                          lmx_depth_diff_t* diffs /* parallel to matches; may be NULL */,
                                          lmx_cluster_t* clusters, size_t cap_clusters, size_t* cluster_offsets, int32_t* members, size_t cap_members);

/* ---- the normal term of the second cluster score ------------------------------------------------------------------------------------------
 * The other half of depth_normal_diff_calc (src/rgbdDetector.cpp:284-359): the mean angle between the surface normals of the template's
 * rendered depth and of the scene depth over the pixels both cover.  The depth term cannot tell a wall at the right distance from the
 * object; this one can.  Definition (csrc/lmx_normal_verify.hpp; the repository's own: the reference takes its normals from OpenCV's rgbd
 * module, RGBD_NORMALS_METHOD_LINEMOD, which is not part of it -- DESIGN.md, deviations):
 *   normal of a pixel   for a uint16-mm image D (reads outside the image or crop give 0): invalid iff d = D[y][x] is 0 or >= distance_threshold;
 *                       else DepthNormal's least squares over the eight taps at offsets +-5 (a tap counts iff |tap - d| < difference_threshold),
 *                       det / ddx / ddy in 64-bit integers as the depth quantiser computes them; nx = (float)fx * (float)ddx,
 *                       ny = (float)fy * (float)ddy, nz = -(float)(det * d); s = sqrtf(nx*nx + ny*ny + nz*nz) without contraction; invalid
 *                       unless s > 0; q_c = (int16)rintf((n_c * (1.0f / s)) * 16384.0f).  Stored as four int16 {qx, qy, qz, valid}, all zeros
 *                       when invalid.  Bit-equal between the CPU build of the header and gfx950.
 *   angle of a pair     integer differences of the stored normals, c2 = dx^2 + dy^2 + dz^2 in 64 bits, c = sqrtf((float)c2),
 *                       i = min(16384, (int)rintf(c * 0.5f)), angle in microradians = table[i], table[i] = llrint(2e6 * asin(min(1, i / 16384.0)))
 *                       (lmx_normal_angle_table: built on the host in double and uploaded; resolution 122 urad; identical normals give 0).
 *   sums of a match     a crop pixel counts iff it counts for the depth term and both normals are valid: n_normal of them, sum_angle_urad
 *                       their angles' sum in 64 bits (order-independent, hence the same for every reduction shape).
 *   value of a match    lmx_match_value = -(sum_abs_mm / (n_valid * 1000.0) + sum_angle_urad / (n_normal * 1e6)) in double, no_value when
 *                       n_valid == 0 or n_normal == 0 (or a NULL argument).  A cluster's score is the mean of it over the members in voting
 *                       order: the logarithm of the reference's 1 / exp(a) * 1 / exp(b), so clusters rank in the same order, and
 *                       exp(score) is the reference's number when every member has something to compare.
 * Template normals are computed on the crop, zero-extended: outside the silhouette the render is 0 anyway; an object that touches the
 * render's border is a documented deviation.
 * enable_normals computes the normals of every crop once (k_normal_map_crops) and keeps them next to the crops; a second call with other
 * parameters recomputes.  lmx_depth_templates_device_bytes then also counts 8 bytes per crop element (rows padded as the depth crops':
 * four times the crops' bytes) and 8 bytes of table per template.  An object that never calls it allocates and launches nothing new.
 * Scene normals are computed once per scene (k_normal_map_frames), when a normal-scored call first needs them, behind the scene's event.
 * fx, fy: focal lengths in pixels, above 0 and at most 1e6 (no float of the normal can overflow); both thresholds >= 1 (upstream's
 * DepthNormal: 50 and 2000). */
typedef struct lmx_normal_params { double fx, fy; int32_t difference_threshold, distance_threshold; } lmx_normal_params;
typedef struct lmx_normal_diff_t { int64_t sum_angle_urad; int32_t n_normal; int32_t reserved; } lmx_normal_diff_t;
lmx_status lmx_normal_angle_table(uint32_t* out /*[16385]*/);
lmx_status lmx_depth_templates_enable_normals(lmx_depth_templates* templates, const lmx_normal_params* params);
/* reads template id's normals back from the device; LMX_ERR_INVALID_ARG before enable_normals */
lmx_status lmx_depth_templates_get_normals(const lmx_depth_templates* templates, int32_t id, int16_t* out /*[h][w][4]*/);
/* lmx_depth_diff_matches with both terms in one pass over each crop (k_walk<NORMALS>): the same arguments, the same staging, the same rule
 * that the uploaded scene is forgotten, the same errors, plus LMX_ERR_INVALID_ARG before enable_normals.  out[i] and, unless it is NULL,
 * ddiffs[i] belong to matches[i]; ddiffs equals what lmx_depth_diff_matches gives, bit for bit. */
lmx_status lmx_normal_diff_matches(lmx_depth_templates* templates, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                                   const size_t* offsets, int32_t class_index, lmx_depth_diff_t* ddiffs /* may be NULL */, lmx_normal_diff_t* out);
double     lmx_match_value(const lmx_depth_diff_t* ddiff, const lmx_normal_diff_t* ndiff, double no_value);
/* lmx_ctx_collect_clusters_depth with both terms:
 *     lmx_ctx_enqueue;  lmx_depth_templates_upload_scene;  lmx_ctx_collect_clusters_depth_normal
 *   ndiffs[i]         = the normal sums of matches[i] (parallel to matches; may be NULL; written when matches is),
 *   clusters[k].score = the mean over the cluster's members, in voting order, of lmx_match_value(diffs[i], ndiffs[i], no_value).
 * On the consumer stream: wait for the scene's event, k_normal_map_frames if the scene has no normals yet, the record form of k_walk<NORMALS>, the
 * third form of k_f2_finalize_cluster, one synchronisation; frames the device chain hands back are finished on the host inside the call.
 * Equal, bit for bit, to lmx_ctx_collect + lmx_normal_diff_matches + per frame lmx_cluster_matches_scored on lmx_match_value.  Every
 * condition of lmx_ctx_collect_clusters_depth holds; LMX_ERR_INVALID_ARG, the enqueue staying outstanding, also before enable_normals. */
lmx_status lmx_ctx_collect_clusters_depth_normal(lmx_ctx* ctx, int32_t n_frames, lmx_depth_templates* templates, int32_t class_index, double no_value,
                                                 lmx_match_t* matches, size_t cap_matches, size_t* match_offsets,
                                                 lmx_depth_diff_t* diffs /* parallel to matches; may be NULL */,
                                                 lmx_normal_diff_t* ndiffs /* parallel to matches; may be NULL */,
                                                 lmx_cluster_t* clusters, size_t cap_clusters, size_t* cluster_offsets, int32_t* members, size_t cap_members);
/* ---- the device chain for a bank of several classes ------------------------------------------------------------------------------------
 * lmx_cluster_matches_classes on the device, from the raw-match slot: one enqueue quantises the frame once for every object of the bank,
 * and the consumer chain votes, filters, scores and suppresses per class.  Stages A - D of k_f2_finalize_cluster (insertion order,
 * std::sort, std::unique: they run over all classes and compare the class already) are shared; the CLASSES forms then pack the class on
 * top of the vote key (class 4 bits | y / step 16 | x / step 16 | ring 17 | list position 11), take step, ring constants, size threshold
 * and side-car from a table of 16 classes, and run the emulated std::sort by score and the greedy NMS on one class's clusters at a time.
 *   lmx_ctx_set_cluster_sidecar_class : class class_index's side-car, validated as by lmx_ctx_set_cluster_sidecar; n_templates == 0 removes
 *     it.  class_index 0 .. 15; beyond that LMX_ERR_INVALID_ARG (lmx_cluster_matches_classes on the host takes any number of classes).
 *     State of its own: the un-classed side-car and its three collect calls are not touched and behave as before.
 *   lmx_ctx_collect_clusters_classes  : lmx_ctx_collect_clusters for the oldest outstanding enqueue (same outputs, same locking) plus
 *     cluster_class[k], the class of clusters[k]; a frame's clusters are class 0's, then class 1's, ...  Matches of a class without a
 *     side-car are listed and belong to no cluster.  score == NULL ranks by mean similarity.  With a score, `templates` holds the crops of
 *     all classes, class c's as templates class_base[c] .. class_base[c + 1] (lmx_depth_templates_append joins per-class objects), its
 *     upload_scene was called after the enqueue, and a cluster's score is the mean of lmx_depth_value (normals == 0; ndiffs is not
 *     written) or lmx_match_value (normals != 0, after enable_normals) over its members.  A match whose template_id is outside its
 *     class's range, or whose class is >= n_classes, gets zero diffs and is never compared with another class's crop.
 *     Equal, bit for bit, to lmx_ctx_collect + per class (lmx_depth_diff_matches / lmx_normal_diff_matches on a per-class object at
 *     class_index = c) + lmx_cluster_matches_classes.  Frames of 2049 .. 16384 records are finished by the classed large-frame
 *     kernels; frames of more than 16384 records, with a template_id outside its class's side-car or a depth ring outside the kernels'
 *     packed range (+-2^16 up to 2048 records, +-2^13 beyond) are finished on the host inside the call.
 *     LMX_ERR_INVALID_ARG, the enqueue staying outstanding: no class side-car set; n_classes outside 1 .. 16; class_base[0] != 0;
 *     class_base[n_classes] != lmx_depth_templates_count; a class's range != its side-car's n_templates (0 without one); and every
 *     condition of lmx_ctx_collect_clusters_depth / _depth_normal on the scene and the normals. */
typedef struct lmx_class_score {
  lmx_depth_templates* templates;
  const int32_t* class_base;   /* [n_classes + 1] */
  int32_t n_classes;
  int32_t normals;             /* 0: the depth term alone */
  double no_value;
} lmx_class_score;
lmx_status lmx_ctx_set_cluster_sidecar_class(lmx_ctx* ctx, int32_t class_index, const double* obj_origin_dists, const int32_t* rects, size_t n_templates,
                                             const lmx_cluster_params* params);
lmx_status lmx_ctx_collect_clusters_classes(lmx_ctx* ctx, int32_t n_frames, const lmx_class_score* score /* NULL: mean similarity */,
                                            lmx_match_t* matches, size_t cap_matches, size_t* match_offsets,
                                            lmx_depth_diff_t* diffs /* parallel to matches; may be NULL */,
                                            lmx_normal_diff_t* ndiffs /* parallel to matches; may be NULL */,
                                            lmx_cluster_t* clusters, int32_t* cluster_class, size_t cap_clusters, size_t* cluster_offsets,
                                            int32_t* members, size_t cap_members);
/* Moves src's templates (crops, table entries, rects) behind dst's: src's template i becomes dst's template count(dst) + i, src is left
 * empty and valid.  Both must live on the same device; both mutexes are taken, in address order.  Nothing is copied on the device.  dst's
 * device table is uploaded again on next use, its crop normals are recomputed on next need if normals are enabled, and a scene uploaded
 * to dst is forgotten: lmx_depth_templates_upload_scene comes before the next scored call. */
lmx_status lmx_depth_templates_append(lmx_depth_templates* dst, lmx_depth_templates* src);
/* ---- all six cluster chains left in device memory ---------------------------------------------------------------------------------------
 * lmx_ctx_export_matches_on with `clusters` for every chain lmx_ctx_collect_clusters* offers: classes (0 the un-classed side-car of
 * lmx_ctx_set_cluster_sidecar, 1 the per-class side-cars of lmx_ctx_set_cluster_sidecar_class) times score (0 mean similarity, 1 the depth
 * score of lmx_ctx_collect_clusters_depth, 2 depth + normal of lmx_ctx_collect_clusters_depth_normal).  For every frame with status 0 the
 * matches, diffs, ndiffs, clusters (score included), cluster_class and members are bit for bit, and in order, what the matching
 * lmx_ctx_collect_clusters* call returns for the same enqueue; classes 0, score 0 equals lmx_ctx_export_matches_on with clusters = 1,
 * header and frame_info included.  Layout, offsets, statuses, header words, capacities of 0 and the ordering rules are those documented
 * there; in addition:
 *   - diffs / ndiffs lie parallel to `matches` and share its capacity and fit decision (a frame's range is written iff its whole match
 *     range fits); cluster_class lies parallel to `clusters_out` and shares the clusters' (and members') decision;
 *   - frames the device chain hands back have status 1 or 2 and counts 0 as there: more than 16384 records, none of max_large_frames
 *     left, a ring outside the packed range, and for classes = 1 a template_id outside its class's side-car.  The enqueue stays
 *     outstanding, so lmx_ctx_collect_clusters_* can still finish them on the host;
 *   - with a score the export stream also waits for the scene's event of `templates` (lmx_depth_templates_upload_scene* after the
 *     enqueue, as for the collect calls), computes the scene's normals first if score = 2 and nobody has (k_normal_map_frames), and walks
 *     the crops of the slot's raw records with k_walk_records_dev: a fixed grid of persistent workgroups that take the record count from
 *     the slot's header on the device.  The object's mutex is held during the call, not until the kernels end: the object records an
 *     event behind the walk instead.  lmx_depth_templates_upload_scene_device makes its copies wait for that event on the device;
 *     lmx_depth_templates_upload_scene, lmx_depth_diff_matches / lmx_normal_diff_matches (when they stage frames), _enable_normals,
 *     _append (both objects) and _free wait for it on the host before they change what the walk reads;
 *   - memory: the first scored call allocates one lmx_depth_diff_t per record the slot can hold (max_batch x max_candidates: 16 B each,
 *     16 MB for 64 frames at the default of 16384 per frame -- the count is not known on the host) and rows of [max_batch][2048] x 48 B;
 *     the first with score = 2 the same again for lmx_normal_diff_t.  A large frame's workspace part is 2.46 MB, 2.72 MB with score 1, 2.98 MB with score 2;
 *   - the first classed scored call, and one whose class_base differs from the previous call's, uploads class_base (a host wait for the
 *     context's earlier exports; no other call waits).
 * Refused before anything is queued, enqueue and context staying usable: everything lmx_ctx_export_matches_on refuses (exactly this
 * struct's size is accepted); everything the matching lmx_ctx_collect_clusters* call refuses -- no side-car(s), templates of another
 * device, a template count or class_base that does not match the side-car(s), score 2 before enable_normals, no scene or one whose
 * frame count or size is not the enqueue's (LMX_ERR_INVALID_ARG), a no_value that is not a number; score outside 0 .. 2 or classes
 * outside 0 .. 1; a null clusters_out or members, a null templates with a score, a null diffs with score >= 1, a null ndiffs with
 * score 2, a null cluster_class or (with a score) class_base with classes; an output that is not plain device memory of the context's
 * device or not aligned to its element (8 bytes for lmx_cluster_t, lmx_depth_diff_t and lmx_normal_diff_t, 4 otherwise).
 * lmx_ctx_chain_stats is not touched: which path a frame took is known on the device alone (frame_info's status, and raw_records > 2048). */
typedef struct lmx_export_clusters_desc {
  uint32_t struct_size;        /* sizeof(lmx_export_clusters_desc) */
  int32_t oldest;              /* as lmx_export_desc */
  int32_t max_large_frames;    /* as lmx_export_desc */
  int32_t classes;             /* 0: the un-classed chain; 1: the per-class chain */
  int32_t score;               /* 0: mean similarity; 1: depth; 2: depth + normal */
  int32_t class_index;         /* classes 0 with a score: as lmx_ctx_collect_clusters_depth takes it (-1: every class) */
  int32_t n_classes;           /* classes 1 with a score: as lmx_class_score */
  int32_t reserved;            /* 0 */
  lmx_depth_templates* templates;   /* score >= 1 */
  const int32_t* class_base;   /* classes 1 with a score: [n_classes + 1], host memory, as lmx_class_score */
  double no_value;             /* score >= 1 */
  uint32_t* header;            /* [16] */
  int32_t* frame_info;         /* [n_frames][8] */
  lmx_match_t* matches;
  size_t cap_matches;
  lmx_depth_diff_t* diffs;     /* score >= 1: parallel to matches */
  lmx_normal_diff_t* ndiffs;   /* score == 2: parallel to matches */
  lmx_cluster_t* clusters_out;
  size_t cap_clusters;
  int32_t* cluster_class;      /* classes == 1: parallel to clusters_out */
  int32_t* members;
  size_t cap_members;
} lmx_export_clusters_desc;
lmx_status lmx_ctx_export_clusters_on(lmx_ctx* ctx, int32_t n_frames, const lmx_export_clusters_desc* desc, void* stream);
/* Test hook: k_walk_records_dev alone, on a slot the caller builds -- a header that says {n_candidates, header_count}, `records` behind it,
 * list capacity `cap`, a grid of grid_workgroups (1 .. 65536) -- against the scene `templates` holds.  class_base NULL: the un-classed
 * predicate with class_index; else the classed one (n_classes + 1 entries ending at the object's template count).  diffs[n_records] and,
 * for both terms, ndiffs[n_records] (NULL: the depth term alone) go to the device as the caller filled them and come back as the kernel
 * left them: entries at or above header_count, and every entry when header_count or n_candidates exceeds cap, keep the caller's bytes.
 * LMX_ERR_INVALID_ARG when a header that did not overflow counts more records than were passed.
 * lmx_debug_depth_walk_grid: the grid lmx_ctx_export_clusters_on launches for this object from now on (0: the default, a multiple of the
 * device's compute units) -- for the measurement in profiles/export_clusters.txt. */
lmx_status lmx_debug_depth_walk_records(lmx_depth_templates* templates, const lmx_raw_match_t* records, size_t n_records, uint32_t header_count,
                                        uint32_t n_candidates, uint32_t cap, int32_t grid_workgroups, int32_t class_index,
                                        const int32_t* class_base, int32_t n_classes, lmx_depth_diff_t* diffs, lmx_normal_diff_t* ndiffs);
lmx_status lmx_debug_depth_walk_grid(lmx_depth_templates* templates, int32_t workgroups);
/* Device time of the object's kernels that run per call: with profiling on, a pair of events surrounds each launch; kernel_time waits for
 * the launches in flight and returns the sum of their times and their number since profiling was switched on.  Off (the default) no
 * event is created or recorded. */
enum { LMX_DT_K_NORMAL_MAP_FRAMES = 0, LMX_DT_K_VERIFY_DIFF_RECORDS = 1, LMX_DT_K_VERIFY_DIFF = 2, LMX_DT_K_DEPTH_DIFF_RECORDS = 3, LMX_DT_K_WALK_RECORDS_DEV = 4, LMX_DT_K_POSE_REFINE = 5, LMX_DT_K_POSE_VERIFY = 6,
       LMX_DT_K_POSE_REFINE_CLUSTERS = 7, LMX_DT_K_POSE_VERIFY_CLUSTERS = 8, LMX_DT_K_SCENE_FILTER_SCORE = 9, LMX_DT_K_SCENE_FILTER_APPLY = 10 };
lmx_status lmx_depth_templates_set_profiling(lmx_depth_templates* templates, int32_t on);
lmx_status lmx_depth_templates_kernel_time(lmx_depth_templates* templates, int32_t kernel, double* total_ms, int64_t* launches);
/* Test hook: the normals of frame `frame` of the uploaded scene as the device holds them (computed now if no call has needed them yet). */
lmx_status lmx_debug_scene_normals(lmx_depth_templates* templates, int32_t frame, int16_t* out /*[H][W][4]*/);

/* ---- pose refinement of matches against the scene depth (the reference's step 7, icpPoseRefine) ------------------------------------------
 * Turns "template i matched at (x, y)" into a rigid transform, on the device, from what the object already holds: the model cloud is
 * template i's depth crop back-projected through the camera it was rendered with, the scene cloud is the scene depth back-projected.
 * The start is the template's own view moved onto the scene by the centroids of the pixels that meet (the reference's
 * getPositionBySurfaceCentroid); then up to max_iterations rounds of: projective association in a (2 search_radius + 1)^2 window, one
 * linearised point-to-point step (6 x 6 Cholesky), quaternion update.  The definition, complete, is the opening comment of
 * csrc/lmx_pose_refine.hpp: integer sums in 1/16 mm, doubles in one written order, no transcendental function; the device (k_pose_refine,
 * one 256-lane workgroup per match, all iterations in one launch) equals the CPU build of that header bit for bit.  PCL is not part of
 * the reference; INTEGRATION.md 3g lists the deviations (no kd-tree, no SVD, no RANSAC rejection).
 * A record maps a point of the template's view (model camera frame, mm) into the scene camera frame: X_scene = R X_view + t_mm. */
enum { LMX_POSE_NONE = 0, LMX_POSE_CONVERGED = 1, LMX_POSE_MAX_ITERATIONS = 2, LMX_POSE_NO_OVERLAP = 3, LMX_POSE_LOST = 4 };
typedef struct lmx_pose_refine_params {
  uint32_t struct_size;
  double model_fx, model_fy, model_cx, model_cy;   /* the camera the crops were rendered with */
  double scene_fx, scene_fy, scene_cx, scene_cy;   /* the depth frame's camera */
  double max_dist_mm, eps_rot_rad, eps_trans_mm;   /* (0, 1024], >= 0, >= 0 */
  int32_t max_iterations, min_pairs, search_radius;  /* 0..64, >= 3, 0..2 */
  const int32_t* rects;                            /* [count][4], NULL: the object's own (lmx_depth_templates_rect) */
} lmx_pose_refine_params;
typedef struct lmx_pose_refine_t {
  double R[9], t_mm[3];
  double rms_first_mm, rms_last_mm;
  int32_t n_model, n_pairs_first, n_pairs_last, iterations, status, reserved;
} lmx_pose_refine_t;
/* The arguments, staging, errors and scene-forgetting rule of lmx_depth_diff_matches; out[i] belongs to matches[i], matches of another
 * class get zeroed records (status LMX_POSE_NONE), as does a match of an empty crop.  depth == NULL: the scene that upload_scene /
 * upload_scene_device left in the object (n_frames must be its frame count); no frame is uploaded again and the scene stays.
 * LMX_ERR_INVALID_ARG before any device work: a wrong struct_size; focal lengths that are NaN, not positive or outside [2^-10, 2^20];
 * principal points outside +-2^20; a parameter outside the range noted above; a rect corner of a selected match outside +-2^17; frames
 * wider or higher than 2^17; depth == NULL without an uploaded scene or with another frame count. */
lmx_status lmx_pose_refine_matches(lmx_depth_templates* templates, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                                   const size_t* offsets, int32_t class_index, const lmx_pose_refine_params* params, lmx_pose_refine_t* out);
/* The object's pose in the scene camera (the reference's it->pose = tf * it->pose): R_obj = R R_view, t_obj_m = (R (0, 0, 1000 distance) + t_mm) / 1000.
 * A pure host function. */
lmx_status lmx_pose_compose(const lmx_mesh_view* view, const lmx_pose_refine_t* refined, double R_obj[9], double t_obj_m[3]);
/* Test hook: one match against one host frame; next to its record the integer sums of every pass the device ran, sums[max_iterations + 1][17]
 * (rows of passes that did not run are zeros); under a schedule sums[sum of the stages' max_iterations + 1][17], in the order the passes ran. */
lmx_status lmx_debug_pose_refine_sums(lmx_depth_templates* templates, const lmx_image* depth, const lmx_match_t* match,
                                      const lmx_pose_refine_params* params, lmx_pose_refine_t* out, int64_t* sums);
/* A refinement schedule: 1 to LMX_POSE_MAX_STAGES stages where lmx_pose_refine_params describes one -- the reference's icpPoseRefine runs a
 * coarse alignment and a fine one that starts from it, over a thinned model cloud.  Every stage has its own correspondence distance,
 * stopping rule, window and a stride in {1, 2, 4, 8}: its passes take only the crop pixels (i, j) with i % stride == 0 and
 * j % stride == 0, and cost in proportion.  A stage starts from the pose the one before it left; all stages run inside the one launch.
 * A stage that is not the last needs max_iterations >= 1 and runs no measuring pass; the last one behaves as a call without a schedule
 * does.  In a record, iterations is the total over the stages, status that of the last stage that ran, and `reserved` the index of the
 * stage that finished it.  The definition is the SCHEDULE paragraph of csrc/lmx_pose_refine.hpp; one stage of stride 1 that repeats the
 * parameters gives the bytes of a call without a schedule.
 * The schedule is a property of the object, like enable_normals; lmx_depth_templates_append keeps the destination's.  While one is set,
 * lmx_pose_refine_matches, lmx_debug_pose_refine_sums, lmx_pose_chain_on, lmx_debug_pose_chain, lmx_rough_pose_chain_on and
 * lmx_debug_rough_pose_chain refine by it: of their lmx_pose_refine_params they take the cameras, min_pairs and rects; max_dist_mm,
 * eps_rot_rad, eps_trans_mm, max_iterations and search_radius are still range-checked but not read.  stages == NULL or n_stages == 0
 * clears it.  The setter waits for nothing: a call reads the schedule on the host and hands it to its kernel by value, so work that is
 * already queued is never affected.  LMX_ERR_INVALID_ARG, the previous schedule staying in place: n_stages outside 0..4; NULL stages with
 * n_stages > 0; a field outside the range lmx_pose_refine_params gives it, or a NaN; another stride; a non-zero `reserved`; a stage in
 * front of the last with max_iterations == 0.  get: the stages set (the rest of out[] zeroed) and their number, 0 for none. */
typedef struct lmx_pose_refine_stage {
  double max_dist_mm, eps_rot_rad, eps_trans_mm;
  int32_t max_iterations, search_radius, stride, reserved;
} lmx_pose_refine_stage;
enum { LMX_POSE_MAX_STAGES = 4 };
lmx_status lmx_depth_templates_set_refine_schedule(lmx_depth_templates* templates, const lmx_pose_refine_stage* stages, int32_t n_stages);
lmx_status lmx_depth_templates_get_refine_schedule(const lmx_depth_templates* templates, lmx_pose_refine_stage out[LMX_POSE_MAX_STAGES], int32_t* n_stages);
/* The point-to-plane metric, per stage and opt-in: a stage with point_shift k in 0..20 minimises the distance of every pair along the
 * scene's stored normal at the pair's scene pixel (the normals of lmx_depth_templates_enable_normals, computed once per scene on the
 * device), kept well-posed by the point-to-point term weighted 2^-k; -1 is the point-to-point stage in every byte.  On flat, box-like
 * parts a few plane passes end where many point passes end, since a model point may slide along the surface; with a small point weight
 * (k >= 8) the pose can wander after about 5 passes, so use it with few iterations.  The definition is the PLANE paragraph of
 * csrc/lmx_pose_refine.hpp.  rms_first_mm / rms_last_mm stay point-to-point distances; the records keep their layout.
 * Entry s governs stage s of whatever schedule is in force; a call without a schedule is stage 0; stages beyond n_stages are -1.
 * point_shift == NULL or n_stages == 0 clears the setting.  Like the schedule it is a property of the object, read on the host by
 * lmx_pose_refine_matches, the pose chains and their hooks and handed to the kernel by value; a call in which no stage in force has a
 * shift >= 0 launches the kernels a call on an object without the setting launches.  LMX_ERR_INVALID_ARG, the previous setting staying in
 * place: n_stages outside 0..4; NULL with n_stages > 0; an entry outside -1..20; an entry >= 0 before lmx_depth_templates_enable_normals.
 * get: all LMX_POSE_MAX_STAGES entries (-1 where none was set) and the number set, 0 for none. */
lmx_status lmx_depth_templates_set_refine_plane(lmx_depth_templates* templates, const int32_t* point_shift, int32_t n_stages);
lmx_status lmx_depth_templates_get_refine_plane(const lmx_depth_templates* templates, int32_t out[LMX_POSE_MAX_STAGES], int32_t* n_stages);
/* Test hook: lmx_debug_pose_refine_sums with the 29 plane sums of every pass next to the 17, plane_sums[the same rows][29]; the rows of
 * passes of a -1 stage, and of passes that did not run, are zeros. */
lmx_status lmx_debug_pose_refine_plane_sums(lmx_depth_templates* templates, const lmx_image* depth, const lmx_match_t* match,
                                            const lmx_pose_refine_params* params, lmx_pose_refine_t* out, int64_t* sums, int64_t* plane_sums);

/* ---- verification of refined poses against the scene's voxel occupancy (the reference's hypothesisVerification) -------------------------
 * The step after icpPoseRefine: the share of the posed model cloud's points that fall into a voxel holding a scene point.  The model
 * cloud is the matched template's crop back-projected and moved by the pose of its lmx_pose_refine_t; the voxels form a lattice of side
 * voxel_mm anchored at the camera origin; the scene points are those of the pixels around the posed model's projection (roi_margin
 * pixels wider on every side, clipped to the image).  At most 2^18 voxels between the extreme model points (a 32 KiB bitmap); a job with
 * more gets LMX_VERIFY_GRID_TOO_LARGE.  The definition, complete, is the opening comment of csrc/lmx_pose_verify.hpp; the device
 * (k_pose_verify, one 256-lane workgroup per match, one launch) equals the CPU build of that header bit for bit.  INTEGRATION.md 3h
 * lists the deviations from PCL's octree. */
enum { LMX_VERIFY_NONE = 0, LMX_VERIFY_OK = 1, LMX_VERIFY_EMPTY = 2, LMX_VERIFY_GRID_TOO_LARGE = 3 };
typedef struct lmx_pose_verify_params {
  uint32_t struct_size;
  double model_fx, model_fy, model_cx, model_cy;   /* the camera the crops were rendered with */
  double scene_fx, scene_fy, scene_cx, scene_cy;   /* the depth frame's camera */
  double voxel_mm;                                 /* [0.25, 64]; the reference uses 4 */
  int32_t roi_margin;                              /* 0..64 pixels */
  const int32_t* rects;                            /* [count][4], NULL: the object's own (lmx_depth_templates_rect) */
} lmx_pose_verify_params;
typedef struct lmx_pose_verify_t {
  double rate;                                     /* n_occupied / n_model (0 without model points) */
  int32_t n_model, n_tested, n_occupied, n_scene;  /* crop pixels != 0; those in front of the camera; those in a marked voxel; scene pixels that marked one */
  int32_t cells, status;                           /* voxels between the extreme tested points, min(.., 2^31 - 1); LMX_VERIFY_* */
  int32_t roi[4];                                  /* x, y, w, h of the scene pixels looked at; zeros: none */
} lmx_pose_verify_t;
/* The arguments, staging, depth == NULL rule, scene-forgetting rule and errors of lmx_pose_refine_matches; poses[i] and out[i] belong to
 * matches[i] (poses: what lmx_pose_refine_matches returned for the same matches; only R and t_mm and status are read).  A match of another
 * class, a match of an empty crop and a match whose pose has status LMX_POSE_NONE get zeroed records (LMX_VERIFY_NONE).
 * LMX_ERR_INVALID_ARG before any device work, next to those of lmx_pose_refine_matches: voxel_mm or roi_margin outside its range; with
 * the match's index in the message, a selected pose with an entry that is not finite, |R[k]| > 2 or |t_mm[k]| > 2^20; frames of more
 * than 2^31 - 1 pixels. */
lmx_status lmx_pose_verify_matches(lmx_depth_templates* templates, const lmx_image* depth, int32_t n_frames, const lmx_match_t* matches,
                                   const size_t* offsets, int32_t class_index, const lmx_pose_refine_t* poses, const lmx_pose_verify_params* params,
                                   lmx_pose_verify_t* out);
/* The reference's erase rule (count / model_pts < thresh erases; 0.3 in the carmine node, 0.2 in the ensenso nodes):
 * keep[i] = status == LMX_VERIFY_OK && !(rate < thresh).  A pure host function. */
lmx_status lmx_pose_verify_keep(const lmx_pose_verify_t* records, size_t count, double thresh, uint8_t* keep);

/* ---- both pose stages on the clusters an export left in device memory ------------------------------------------------------------------
 * What lmx_ctx_export_matches_on (clusters = 1) or lmx_ctx_export_clusters_on wrote goes in; per exported cluster slot k the leader match
 * (the member of highest similarity, the first on a tie: its index into `matches`), its lmx_pose_refine_t, its lmx_pose_verify_t and the
 * keep decision of lmx_pose_verify_keep come out, in the caller's device arrays parallel to `clusters`, with no host wait in between: the
 * counterpart, for a pipelined caller, of reading the clusters back, picking the leaders and calling lmx_pose_refine_matches and
 * lmx_pose_verify_matches with depth == NULL -- and bit for bit what those return for the same lists and resident scene.  No arithmetic
 * of its own: csrc/lmx_pose_refine.hpp and csrc/lmx_pose_verify.hpp define the records, csrc/lmx_pose_chain.hpp what is decided from the
 * lists (k_pose_refine_clusters, k_pose_verify_clusters: one workgroup per slot, a grid of cap_clusters, three launches per call).
 *   n_live = min(header[3], cap_clusters).  Slots at or above it are not written.  A slot below it whose frame has a status other than 0,
 *   or a range beyond one of this call's capacities, is dead: leader -1, zeroed records, keep 0.  Every index read from device memory is
 *   checked before it is used as an address: a cluster without members, a member range beyond min(header[4], cap_members), a member outside
 *   its frame's matches (leader -1), a template_id outside the table -- with class_base a class outside [0, n_classes) or an id outside
 *   its class's range --, a rect corner beyond +-2^17 (the leader's index) give zeroed records and flag 2.  A leader of another class than
 *   class_index gets zeroed records, as in the host calls.  A refined pose that lmx_pose_verify_matches would refuse (an entry not finite,
 *   |R| > 2, |t_mm| > 2^20) gets a zeroed verify record and flag 4.
 *   chain_header[8]: [0] n_live, [1] flags (1: the export's list overflowed, or a capacity -- the export's or this call's -- cut live
 *   slots; 2; 4), [2] slots whose pose status is not LMX_POSE_NONE, [3] slots verified LMX_VERIFY_OK, [4] slots kept, rest 0.
 * The scene is the resident one (lmx_depth_templates_upload_scene / _device); n_frames must be its frame count.
 * Ordering (`stream`: the HIP stream the export was given and that will consume the results; NULL = the null stream), as
 * lmx_ctx_export_clusters_on: the kernels run on the object's own stream, which waits ON THE DEVICE for what `stream` holds at the call
 * (the export made it wait for its own end) and for the scene's copies; before returning, `stream` is made to wait for the chain's end;
 * every call that replaces or frees what the kernels read (the scene, the crops, the table) waits for them as it waits for an export's
 * walk; nothing is waited for or read on the host.  The rects of both parameter sets and class_base are uploaded on the first call and
 * when they differ from the previous call's (that upload waits for the previous chain).
 * Refused before anything is queued with LMX_ERR_INVALID_ARG: a struct_size other than the struct's (the desc's or either params');
 * everything lmx_pose_refine_matches and lmx_pose_verify_matches refuse of their parameters; a null input or output; an array that
 * hipPointerGetAttributes does not report as plain device memory of the object's device, or that is not aligned to its element (8 bytes
 * for clusters, poses and checks, 1 for keep, 4 otherwise); cap_clusters 0 or above 2^20; n_frames < 1; no resident scene or one of another
 * frame count; a class_base that does not start at 0, decreases or does not end at the object's template count; a keep_thresh that is NaN;
 * a `stream` that is being captured. */
typedef struct lmx_pose_chain_desc {
  uint32_t struct_size;            /* sizeof(lmx_pose_chain_desc) */
  int32_t n_frames;
  int32_t class_index;             /* as lmx_pose_refine_matches; ignored with class_base */
  int32_t n_classes;               /* with class_base */
  const int32_t* class_base;       /* host, [n_classes + 1], as lmx_class_score; NULL: template_id indexes the table directly */
  const lmx_pose_refine_params* refine;
  const lmx_pose_verify_params* verify;
  double keep_thresh;              /* the reference: 0.3 carmine, 0.2 ensenso */
  /* inputs: what the export wrote, device memory */
  const uint32_t* header;          /* [16] */
  const int32_t* frame_info;       /* [n_frames][8] */
  const lmx_match_t* matches;
  size_t cap_matches;
  const lmx_cluster_t* clusters;
  size_t cap_clusters;
  const int32_t* members;
  size_t cap_members;
  /* outputs, device memory, [cap_clusters] each, parallel to `clusters` */
  uint32_t* chain_header;          /* [8] */
  int32_t* leaders;
  lmx_pose_refine_t* poses;
  lmx_pose_verify_t* checks;
  uint8_t* keep;
} lmx_pose_chain_desc;
lmx_status lmx_pose_chain_on(lmx_depth_templates* templates, const lmx_pose_chain_desc* desc, void* stream);
/* Test hook: the same two kernels on lists in HOST memory.  Every pointer of `desc` but class_base and the parameters' is a host array
 * of the stated capacity (header [16], frame_info [n_frames][8], chain_header [8]; a capacity of 0: the array is not looked at); the five
 * inputs are uploaded, the five outputs go to the device as they are and come back as the kernels left them: entries the kernels did
 * not write keep the caller's bytes (chain_header is zeroed by the call itself). */
lmx_status lmx_debug_pose_chain(lmx_depth_templates* templates, const lmx_pose_chain_desc* desc);

/* ---- rough pose per cluster: mean view of the largest orientation group, the model rendered again ---------------------------------------
 * The reference's getRoughPoseByClustering (src/rgbdDetector.cpp:586-865) in front of the two pose stages, where lmx_pose_chain_on takes
 * the cluster's leader and its stored crop.  Per exported cluster slot: the members are grouped by the orientation of their views (first
 * fit in member order against the member that created each group; two views are the same when the trace of R_a^T R_b exceeds trace_min
 * = 1 + 2 cos(threshold), lmx_rough_trace_min); the largest group wins (what std::sort by size leaves first); its views' quaternions,
 * distances, D and ori_dist and its matches' positions are averaged; the mesh is rendered at that mean view (the arithmetic of
 * lmx_mesh_render, bit for bit) into the slot's window of the model object; that render, placed with the corner of its silhouette box at
 * the mean position, is refined and verified as lmx_pose_refine_matches and lmx_pose_verify_matches would a stored crop of the same pixels.
 * The definition, complete, is the opening comment of csrc/lmx_rough_pose.hpp; the device equals the CPU build of that header bit for
 * bit.  INTEGRATION.md 3j lists the deviations from the reference.  One mesh and one view table per call: several objects with a
 * class_base, as lmx_pose_chain_on has it, are deliberately out of scope -- call once per class with class_index.
 *
 * The model object holds in device memory the mesh, the view table (views[i] belongs to template_id i of the matches; D and ori_dists:
 * the side-car's, NULL: zeros) and per slot a view, the rasteriser's state, a work row of n_triangles records (96 bytes each), a depth
 * window of max_window_h rows of max_window_w pixels (rows padded to 16 bytes) and a crop table entry: lmx_rough_model_device_bytes says
 * how much.  LMX_ERR_INVALID_ARG: what lmx_mesh_render refuses of a mesh, a camera and views; n_views < 1; a view whose R^T R - I has an
 * entry beyond 1e-6; a D or ori_dist that is not finite; cap_slots outside 1 .. 2^16; a window side outside 1 .. the camera's.
 * A model serves the calls of any lmx_depth_templates object of its device, one after the other (each call's stream waits for the previous
 * call's end on the device); lmx_rough_model_free waits for the device. */
typedef struct lmx_rough_model lmx_rough_model;
lmx_status lmx_rough_model_create(int32_t device, const double* triangles /*[n][3][3] m*/, int32_t n_triangles, const lmx_mesh_camera* cam,
                                  const lmx_mesh_view* views, int32_t n_views, const double* D /*[n_views], NULL ok*/,
                                  const double* ori_dists /*[n_views], NULL ok*/, int32_t cap_slots, int32_t max_window_w, int32_t max_window_h,
                                  lmx_rough_model** out);
void lmx_rough_model_free(lmx_rough_model* model);
size_t lmx_rough_model_device_bytes(const lmx_rough_model* model);
/* trace_min = 1 + 2 cos(degrees pi / 180) for an angle inside (0, 180); anything else: LMX_ERR_INVALID_ARG.  A pure host function. */
lmx_status lmx_rough_trace_min(double degrees, double* trace_min);

enum { LMX_ROUGH_NONE = 0, LMX_ROUGH_OK = 1, LMX_ROUGH_TOO_MANY_GROUPS = 2, LMX_ROUGH_DEGENERATE = 3, LMX_ROUGH_INVALID_VIEW = 4,
       LMX_ROUGH_WINDOW_TOO_LARGE = 5, LMX_ROUGH_EMPTY = 6 };
/* R, distance: the mean view, an lmx_mesh_view for lmx_pose_compose.  x, y: the mean match position (truncating integer means).  front:
 * the index into `matches` of the member that created the winning group; group: its index in creation order.  rect: x, y, w, h of the
 * render's silhouette box in the model camera; n_model: its covered pixels.  Status: TOO_MANY_GROUPS more than 512 groups (n_members and
 * n_groups = 512 set, the rest zero); DEGENERATE the quaternion sum has a squared norm of 0 or not finite (R zeros); INVALID_VIEW the mean
 * view puts a vertex at Z <= 0.01; WINDOW_TOO_LARGE the union of the triangles' boxes exceeds the model's window; EMPTY no pixel is
 * covered.  rect and n_model are zeros unless the status is OK. */
typedef struct lmx_rough_pose_t {
  double R[9], distance, D, ori_dist;
  int32_t x, y, n_members, n_groups, group, n_group_members, front, center_hole;
  int32_t rect[4];
  int32_t n_model, status;
} lmx_rough_pose_t;
/* lmx_pose_chain_desc without class_base and n_classes, with trace_min, `rough` in place of `leaders` and member_group, parallel to
 * `members`: the group (creation order) of every member of a slot whose members passed the index checks, -1 from the member on that
 * would have created group 513.  refine->rects and verify->rects must be NULL: the rects are the rendered ones.
 *   Slots, n_live, dead slots and the flags 1, 2 and 4 as lmx_pose_chain_on.  Checked before any value is used as an address, flag 2 and
 *   an all-zero rough record each: a member outside its frame's matches; a member of another class than the first member's; a template_id
 *   outside [0, n_views); a mean position beyond +-2^17.  With class_index >= 0 a first member of another class gives an all-zero record
 *   and no flag.  A slot whose rough status is not LMX_ROUGH_OK gets zeroed pose and verify records and keep 0.
 *   chain_header[8]: as lmx_pose_chain_on's, plus flag 8 (a slot that passed the checks ended with a rough status other than OK) and
 *   [5] the slots of status LMX_ROUGH_OK.
 * Ordering, the resident scene, the pointer and parameter checks are those of lmx_pose_chain_on (rough: 8-byte aligned, member_group: 4).
 * Refused in addition, with LMX_ERR_INVALID_ARG before anything is queued: a model of another device; cap_clusters above the model's
 * cap_slots; a model camera whose fx, fy, cx, cy differ from the model_* of either parameter set; a trace_min that is NaN; rects that
 * are not NULL.  Six kernel launches per call, no host wait. */
typedef struct lmx_rough_chain_desc {
  uint32_t struct_size;            /* sizeof(lmx_rough_chain_desc) */
  int32_t n_frames;
  int32_t class_index;             /* >= 0: only clusters whose first member has this class; -1: every cluster */
  int32_t reserved;
  const lmx_pose_refine_params* refine;
  const lmx_pose_verify_params* verify;
  double keep_thresh;
  double trace_min;                /* lmx_rough_trace_min(threshold in degrees) */
  const uint32_t* header;          /* [16] */
  const int32_t* frame_info;       /* [n_frames][8] */
  const lmx_match_t* matches;
  size_t cap_matches;
  const lmx_cluster_t* clusters;
  size_t cap_clusters;
  const int32_t* members;
  size_t cap_members;
  /* outputs, device memory */
  uint32_t* chain_header;          /* [8] */
  lmx_rough_pose_t* rough;         /* [cap_clusters] */
  int32_t* member_group;           /* [cap_members] */
  lmx_pose_refine_t* poses;        /* [cap_clusters] */
  lmx_pose_verify_t* checks;       /* [cap_clusters] */
  uint8_t* keep;                   /* [cap_clusters] */
} lmx_rough_chain_desc;
lmx_status lmx_rough_pose_chain_on(lmx_depth_templates* templates, lmx_rough_model* model, const lmx_rough_chain_desc* desc, void* stream);
/* Test hook: the same kernels on lists in HOST memory, staged exactly as lmx_debug_pose_chain stages them: the five inputs are uploaded,
 * the six outputs go to the device as they are and come back as the kernels left them (chain_header is zeroed by the call itself). */
lmx_status lmx_debug_rough_pose_chain(lmx_depth_templates* templates, lmx_rough_model* model, const lmx_rough_chain_desc* desc);
/* Test hook: the render the last call left in `slot`, cut to its silhouette box: out [rect[3]][rect[2]] (room for max_window_w *
 * max_window_h elements), rect = x, y, w, h in the model camera; zeros and nothing written for a slot without a render.  Waits for the
 * device. */
lmx_status lmx_debug_rough_crop(lmx_rough_model* model, int32_t slot, uint16_t* out, int32_t rect[4]);

/* ---- depth outlier filter of the scene ahead of the pose stages (the reference's statisticalOutlierRemoval) ----------------------------------
 * The reference cleans every cluster's scene cloud with statisticalOutlierRemoval(scene_pc, 50, 1.0) (src/rgbdDetector.cpp:836) before it
 * takes the surface centroid, runs ICP and checks the occupancy: the flying pixels a structured-light or stereo sensor leaves on depth
 * discontinuities would otherwise enter all three.  This is that step as an opt-in property of a lmx_depth_templates object.  While it is
 * set, lmx_pose_refine_matches, lmx_pose_verify_matches, lmx_pose_chain_on, lmx_rough_pose_chain_on and their debug hooks
 * (lmx_debug_pose_refine_sums, lmx_debug_pose_refine_plane_sums, lmx_debug_pose_chain, lmx_debug_rough_pose_chain) read a filtered copy of
 * the scene -- the resident one or the frames staged from `depth` alike -- in which every outlier pixel is 0, "no measurement", which the
 * stages already skip.  The depth and normal cluster scores and the stored scene normals of the point-to-plane metric keep the raw scene.
 * An object on which it was never set launches the kernels it launched before, with the same arguments.
 *   The definition, complete, is the opening comment of csrc/lmx_scene_filter.hpp: for every valid pixel the mean distance to its k nearest
 * of the (2 radius + 1)^2 window neighbours, over the pixel's own depth; a pixel with fewer than k neighbours within 1024 mm is removed as
 * sparse; of the others, those whose score exceeds the frame's mean + stddev_mul standard deviations are removed.  Integer sums, a threshold
 * formed on the device: the filtered copy is made once per scene, on the object's stream, when a pose stage first needs it, with nothing
 * waited for on the host, and the device equals the CPU build of the header in every byte.  PCL is not part of the reference;
 * INTEGRATION.md 3k and DESIGN.md section 7 list the deviations (window for kd-tree, frame-wide normalised statistics, convex corners with
 * fewer than k same-surface neighbours, no voxel grid).
 *   lmx_scene_filter_defaults fills struct_size, radius 3, k 15, stddev_mul 1.0 and a camera of zeros, which the caller must replace.
 * lmx_depth_templates_set_scene_filter(t, NULL) turns the filter off.  A new setting (or NULL) takes effect with the next call; the copy is
 * computed again.  Refused with LMX_ERR_INVALID_ARG, the previous setting left in place: a struct_size that is not
 * sizeof(lmx_scene_filter_params); radius outside 1..7; k outside 1..(2 radius + 1)^2 - 1; stddev_mul outside [0, 16] or not a number;
 * fx, fy, cx or cy not finite or not above 0; reserved != 0.  The camera is NOT compared with the scene camera of a later call's
 * parameters: it is the caller's to pass the same one.  While the filter is set, the calls above refuse frames of more than 2^22 pixels
 * (the frame's 64-bit sums hold that many scores). */
typedef struct lmx_scene_filter_params {
  uint32_t struct_size;
  int32_t radius, k, reserved;   /* 1..7, 1..(2 radius + 1)^2 - 1, 0 */
  double stddev_mul;             /* [0, 16] */
  double fx, fy, cx, cy;         /* the depth frame's camera */
} lmx_scene_filter_params;
typedef struct lmx_scene_filter_info {   /* one frame's record, 56 bytes */
  int64_t n_valid, n_sparse, n_scored, n_removed;   /* n_valid = n_sparse + n_scored; n_removed of the scored pixels exceed the threshold */
  int64_t sum_q, sum_qq;                            /* over the scored pixels */
  double threshold;                                 /* 2^20 for a frame with fewer than two scored pixels */
} lmx_scene_filter_info;
lmx_status lmx_scene_filter_defaults(lmx_scene_filter_params* out);
lmx_status lmx_depth_templates_set_scene_filter(lmx_depth_templates* templates, const lmx_scene_filter_params* params);
/* Test hook: the filtered copy of frame `frame` of the uploaded scene as the device holds it (computed now if no call has needed it yet) and
 * the frame's record (out_info may be NULL).  LMX_ERR_INVALID_ARG without the setting or without a scene.  Waits for the device. */
lmx_status lmx_debug_scene_filtered(lmx_depth_templates* templates, int32_t frame, uint16_t* out /*[H][W]*/, lmx_scene_filter_info* out_info);

/* ---- introspection (stage-level parity tests, profiling) ------------------------------------------------- */
enum {
  LMX_DBG_QUANTIZED = 0,     /* u8 [H_l][W_l] one-hot labels after quantize(), A.2/A.4 */
  LMX_DBG_LINEAR_MEMORY = 1, /* u8 [8][T*T][W'H'] in upstream linearize() layout, A.7 */
  LMX_DBG_PYRAMID_BGR = 2,   /* u8 [H_l][W_l][3] colour source at level l (pyrDown chain), A.3; [H_l][W_l] on a gray context */
  LMX_DBG_DEPTH = 3,         /* u16 [H][W] level-0 depth in mm as the DepthNormal modality sees it */
  /* Whole device allocations as they are, pads and tails included, every frame of the context: frame must be 0, nothing is launched or
   * written.  A buffer that is too small is refused and the error text names the size. */
  LMX_DBG_RAW_SPREAD = 4,    /* level < L-1: the spread image of (level, modality), max_batch * ls_stride + 8192 bytes */
  LMX_DBG_RAW_NIBBLES = 5,   /* the coarsest level's nibble memories of all modalities, M * max_batch * nib_mod_stride + 8192 bytes (level, modality ignored) */
  LMX_DBG_RAW_BYTES = 6      /* the coarsest level's byte-wide memories of `modality`, max_batch * mod_stride + 8192 bytes; they exist only where
                                the spread kernel does not write nibbles itself (LMX_ERR_INVALID_ARG otherwise) */
};
lmx_status lmx_ctx_debug_read(lmx_ctx* ctx, int32_t frame, int32_t what, int32_t level, int32_t modality, void* out,
                              size_t out_bytes);
/* Test hook: an enqueue whose chain starts at the LABEL IMAGES instead of the uploaded frames.  labels[l * n_modalities + m] is a host array
 * u8 [n_frames][H_l][W_l] (packed, H_l = height >> l, W_l = width >> l) that is copied as it is into the context's label image of (level l,
 * modality m) on the enqueue's stream; then the spread / linearise launches of every level, scoring, refinement and the read-back run as
 * lmx_ctx_enqueue (thresholds null: `threshold` for every class) or lmx_ctx_enqueue_thresholds (thresholds[k] for class index k, `threshold`
 * not read) launch them for n_frames: one or two frames of a two-level bank take the fused spread kernel of the one-frame call where it
 * exists, everything else goes level by level.  No quantiser, pyramid or mask kernel runs; the slot's header and candidate counters, which
 * the first quantiser clears otherwise, are cleared by a memset in stream order.  Always eager, also on a LMX_CTX_HIPGRAPH context, and no
 * upload is needed.  The slot accounting is an enqueue's: lmx_ctx_collect*, lmx_ctx_export_raw, lmx_ctx_release and lmx_ctx_stats follow as
 * usual, and lmx_ctx_debug_read returns the label images and memories of the call.  Any byte is accepted as a label (the quantisers write
 * 0 or one bit).  The arrays must stay valid until the enqueue has been collected or released.
 * LMX_ERR_INVALID_ARG: n_labels != levels * modalities, a null entry, n_frames outside [1, max_batch], a thresholds array that
 * lmx_ctx_enqueue_thresholds would refuse, or as many enqueues outstanding as the context has slots. */
lmx_status lmx_ctx_debug_enqueue_labels(lmx_ctx* ctx, int32_t n_frames, const uint8_t* const* labels, int32_t n_labels, float threshold,
                                        const float* thresholds, int32_t n_thresholds, const char* const* class_ids, int32_t n_class_ids);
/* Test hook: the counters of the context's helper thread (the one-frame lmx_match / lmx_match_batch with host frames hands the rest of its
 * chain to it; csrc/lmx_launch_helper.hpp).  out = {jobs run, times the helper went to sleep, wake-ups sent}: jobs - wake-ups is about the
 * number of calls that found the helper still spinning.  All zero while the context has had no such call (it has no helper thread then) or
 * when the path is switched off.  Call it between matches, from the thread that matches. */
lmx_status lmx_debug_launch_helper_counters(lmx_ctx* ctx, uint64_t out[3]);
/* Test hook for the float stage: the 16-bin orientation label (0..16, before upstream's '& 7') the device code assigns to
 * n gradients (dx[i], dy[i]) -- fastAtan2 in degrees, times 16/360, round half to even. */
lmx_status lmx_debug_orientation_labels(int32_t device, const int16_t* dx, const int16_t* dy, size_t n, uint8_t* out);
/* Test hook for the depth path's float stage: the median bin BEFORE the 5x5 median (0 = no label, k + 1 = label 1 << k) that the depth
 * quantiser's device code gives n tap tuples.  taps: n x 9 values, the pixel's depth d and then its eight neighbours at distance 5 in the
 * order (dy, dx) = (-5,-5) (-5,0) (-5,5) (0,-5) (0,5) (5,-5) (5,0) (5,5); any values, a tuple need not come from an image.  variant picks the
 * code: the int32 form (what a context runs for difference_threshold <= 200), the 64-bit form (larger thresholds), or the int32 form's
 * look-up as the pipelined loop of interior tiles does it.  The int32 variants refuse difference_threshold > 200 (LMX_ERR_INVALID_ARG).
 * normal_lut: 8000 labels as lmx_bank_set_normal_lut takes them, or NULL for the default table. */
enum { LMX_DBG_DEPTH_INT = 0, LMX_DBG_DEPTH_INT64 = 1, LMX_DBG_DEPTH_PIPELINED = 2 };
lmx_status lmx_debug_depth_normal_bins(int32_t device, const uint16_t* taps, size_t n, int32_t distance_threshold, int32_t difference_threshold,
                                       int32_t variant, const uint8_t* normal_lut, uint8_t* out_bins);
/* Test hooks: the permutation produced by the library's restatement of libstdc++'s std::sort (csrc/lmx_sort_emul.hpp, the code the
 * device runs to reproduce upstream's order of ties) for Match::operator< and for the clusters' score-descending comparator. */
lmx_status lmx_debug_introsort_perm(const float* similarity, const int32_t* template_id, int32_t n, int32_t* perm);
lmx_status lmx_debug_introsort_perm_score(const double* score, int32_t n, int32_t* perm);
/* The permutation the DEVICE's workgroup-parallel form of the same algorithm (csrc/lmx_sort_block.hpp, what k_f2_finalize_cluster runs
 * for Detector::match's std::sort) produces for n <= 2048 (similarity, template_id) pairs: must equal lmx_debug_introsort_perm's. */
lmx_status lmx_debug_device_sort_perm(int32_t device, const float* similarity, const int32_t* template_id, int32_t n, int32_t* perm);
/* Test hook: the device consumer chain of lmx_ctx_collect_clusters (k_f2_finalize_cluster, csrc/lmx_f2.hip: the same kernel, the same
 * launch) on records the CALLER supplies instead of a slot an enqueue wrote.  Stand-alone, no context: the records are copied to the
 * device behind a slot header that counts n_records, the slot's capacity is n_records.  A record belongs to frame `frame`; records
 * whose frame is outside 0 .. n_frames - 1 are ignored, frames may be interleaved in any order, order_key must be unique per frame.
 * Outputs (host arrays, all required): matches [n_frames][2048], clusters [n_frames][2048], members [n_frames][2048] and
 * counts [n_frames][4] = {final matches, clusters, members, status}, exactly as the kernel wrote them -- NO host completion:
 *   status 0: the frame is complete; members index the frame's matches, member_begin is relative to the frame's members row;
 *   status 1: more than 2048 records; counts[0] = the frame's record count, nothing else is written;
 *   status 2: a template_id outside the side-car, or a vote bin outside +-2^16 / a depth ring outside +-2^18; counts[0] = final
 *             matches, the frame's matches row is valid, no clusters.
 * (lmx_ctx_collect_clusters finishes status 1 and 2 frames on the host.)  Parameters and side-car are validated as by
 * lmx_ctx_set_cluster_sidecar; n_frames must be 1..8.  Every record's x and y must fit an int16 and its class_index a uint16
 * (LMX_ERR_INVALID_ARG otherwise): the kernel holds them in LDS at that width, which the records of an enqueue always satisfy
 * (image coordinates, class slots).  LMX_ERR_NO_DEVICE without a GPU. */
lmx_status lmx_debug_device_finalize_cluster(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                             const double* obj_origin_dists, const int32_t* rects, size_t n_templates,
                                             const lmx_cluster_params* params, lmx_match_t* matches, lmx_cluster_t* clusters, int32_t* members,
                                             uint32_t* counts);
/* The same hook for the scored form (lmx_ctx_collect_clusters_depth): depth[n_frames] becomes templates' uploaded scene, then
 * the record form of k_walk and the depth-scored k_f2_finalize_cluster run on the stand-alone slot.  diffs [n_frames][2048] comes back next to matches
 * (a frame's row is valid where its matches row is); everything else as above, again without host completion.  templates need not hold
 * n_templates crops: a record whose template_id it does not hold gets a zero diff. */
lmx_status lmx_debug_device_finalize_cluster_depth(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                   lmx_depth_templates* templates, const lmx_image* depth, int32_t class_index, double no_value,
                                                   const double* obj_origin_dists, const int32_t* rects, size_t n_templates,
                                                   const lmx_cluster_params* params, lmx_match_t* matches, lmx_depth_diff_t* diffs,
                                                   lmx_cluster_t* clusters, int32_t* members, uint32_t* counts);
/* The same hook for the CLASSES forms (lmx_ctx_collect_clusters_classes): `classes` as lmx_cluster_matches_classes takes them, n_classes
 * 1 .. 16, each validated as by lmx_ctx_set_cluster_sidecar_class.  score == NULL: the CLASSES form of k_f2_finalize_cluster.  With a score: depth
 * [n_frames] becomes score->templates' uploaded scene, then the classed record kernel and the scored (normals == 0) or normal-scored
 * classed chain; class_base is validated against the object's count only, so that a test can give a class a shorter range than its
 * side-car.  cluster_class [n_frames][2048] comes back next to clusters, diffs and ndiffs [n_frames][2048] next to matches (required with
 * a score / with normals).  Status 2: a template_id outside its class's side-car or a depth ring outside +-2^16.  No host completion. */
lmx_status lmx_debug_device_finalize_cluster_classes(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                     const lmx_class_sidecar* classes, int32_t n_classes, const lmx_class_score* score,
                                                     const lmx_image* depth, lmx_match_t* matches, lmx_depth_diff_t* diffs,
                                                     lmx_normal_diff_t* ndiffs, lmx_cluster_t* clusters, int32_t* cluster_class, int32_t* members,
                                                     uint32_t* counts);
/* Test hook, no device needed: one of the tables a context of width x height frames, max_batch frames per batch and shard
 * shard_rank of shard_world (1: the whole bank) would put on the device for `bank` -- the bytes DeviceBankView's pointers see
 * (csrc/lmx_bank_tables.hpp defines every format); ls_flat != 0 as under LMX_LS_FLAT.  LMX_TAB_SUMMARY is uint32 words:
 * {G, nf_max_coarse, uni_ok, uni_mod_block_bytes, L, M, classes, 0}, then 16 words per pyramid level {W, H, T, Wc, Hc, cells,
 * ori_stride, mod_stride, zero_off, nib_ori_stride, nib_mod_stride, nib_zero_off, ls_stride, ls_zero_off, ls_bands, ls_band_stride}.
 * *n_bytes = the table's size, *fnv1a = the 64-bit FNV-1a hash of its bytes (either may be NULL); out may be NULL to ask for those
 * alone, else out_bytes must hold the table.  Geometry errors are reported as lmx_ctx_create reports them. */
enum { LMX_TAB_INFO = 0, LMX_TAB_LINFO, LMX_TAB_COARSE_OFF, LMX_TAB_COARSE_UNI, LMX_TAB_COARSE_BLK, LMX_TAB_SINFO, LMX_TAB_FEAT, LMX_TAB_FEAT_COUNT, LMX_TAB_SUMMARY };
lmx_status lmx_debug_bank_tables(const lmx_bank* bank, int32_t width, int32_t height, int32_t max_batch, int32_t shard_rank, int32_t shard_world,
                                 int32_t ls_flat, int32_t table, void* out, size_t out_bytes, size_t* n_bytes, uint64_t* fnv1a);
/* The large-frame form of the four hooks above: the kernels lmx_ctx_collect_clusters* launch for the frames the LDS kernels hand back
 * (k_f2_large, csrc/lmx_f2.hip: one workgroup of 1024 threads per frame, rows in device memory), here on EVERY frame whatever its size, with
 * the same arguments and no host completion.  Rows are [n_frames][16384].  Exactness: for every frame of at most 16384 records the outputs
 * equal the reference chain's bit for bit, as the LDS kernels' do -- the same permutation of ties from both sorts, the same double sums.
 *   status 0: complete;   status 1: more than 16384 records, counts[0] = the record count, nothing else written;
 *   status 2: a template_id outside the side-car or a depth ring outside the packed vote key: un-classed -2^17 .. 2^17 - 1, classed
 *             -2^13 .. 2^13 - 1 (the 14-bit list position takes the bits; vote bins y / step, x / step are 16 bits each and always fit);
 *             counts[0] = final matches, the matches row is valid, no clusters.
 * lmx_debug_device_sort_perm_large: the permutation of the big sort for n <= 16384 pairs (n > 16384: LMX_ERR_INVALID_ARG); inputs that
 * exhaust the introsort's depth limit are heap-sorted on the device like the LDS kernel's, so the permutation is std::sort's for them too. */
lmx_status lmx_debug_device_sort_perm_large(int32_t device, const float* similarity, const int32_t* template_id, int32_t n, int32_t* perm);
lmx_status lmx_debug_device_finalize_cluster_large(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                   const double* obj_origin_dists, const int32_t* rects, size_t n_templates,
                                                   const lmx_cluster_params* params, lmx_match_t* matches, lmx_cluster_t* clusters,
                                                   int32_t* members, uint32_t* counts);
lmx_status lmx_debug_device_finalize_cluster_large_depth(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                         lmx_depth_templates* templates, const lmx_image* depth, int32_t class_index,
                                                         double no_value, const double* obj_origin_dists, const int32_t* rects,
                                                         size_t n_templates, const lmx_cluster_params* params, lmx_match_t* matches,
                                                         lmx_depth_diff_t* diffs, lmx_cluster_t* clusters, int32_t* members, uint32_t* counts);
lmx_status lmx_debug_device_finalize_cluster_large_classes(int32_t device, const lmx_raw_match_t* records, size_t n_records, int32_t n_frames,
                                                           const lmx_class_sidecar* classes, int32_t n_classes, const lmx_class_score* score,
                                                           const lmx_image* depth, lmx_match_t* matches, lmx_depth_diff_t* diffs,
                                                           lmx_normal_diff_t* ndiffs, lmx_cluster_t* clusters, int32_t* cluster_class,
                                                           int32_t* members, uint32_t* counts);
/* Counters of the last collect(): coarse candidates and refined matches summed over frames. */
lmx_status lmx_ctx_stats(lmx_ctx* ctx, int64_t* n_candidates, int64_t* n_raw_matches);
/* Which path completed the frames of the last lmx_ctx_collect_clusters, _depth, _depth_normal or _classes call.  A frame of at most 2048
 * raw records is completed by the LDS kernel, one of 2049 .. 16384 by the large-frame kernel (unless the context was created with
 * LMX_F2_LARGE=0 in the environment), a larger one by the host; a frame with a template_id outside its side-car or a depth ring outside a
 * kernel's packed range (the large kernel's is narrower, see the hooks above) is completed by the host whatever its size.  The result is
 * the reference's on every path.  max_frame_records: the largest raw record count among the frames beyond 2048 records, 0 if there was
 * none (the LDS kernel does not report the raw count of a frame it completes).  large_workspace_bytes: the device memory the context
 * holds for the large-frame kernel -- 0 until its first large frame, then one workspace part of 2.46 MB (2.72 MB with the depth score, 2.98 MB
 * with both) per large frame of the busiest call so far. */
typedef struct lmx_chain_stats {
  int32_t frames;               /* frames of the call */
  int32_t frames_lds;           /* completed by the LDS kernel */
  int32_t frames_large;         /* completed by the large-frame kernel */
  int32_t frames_host_records;  /* completed by the host because of their record count */
  int32_t frames_host_other;    /* completed by the host for side-car or range reasons */
  int32_t max_frame_records;
  int64_t large_workspace_bytes;
} lmx_chain_stats;
lmx_status lmx_ctx_chain_stats(lmx_ctx* ctx, lmx_chain_stats* out);

/* Per-kernel HIP-event timing on the context's stream (off by default).  `enabled` is a bitmask over kernel ids
 * (bit k = time kernel k; -1 = all): every timed launch costs two event records, so time only what is reported. */
int32_t lmx_num_kernels(void);
const char* lmx_kernel_name(int32_t kernel_id);
/* Name of the device kernel this context launches for a kernel id (what a profiler shows), e.g. "k_score_coarse_u8" for
 * LMX kernel id "k_score_coarse" when every template has <= 63 coarsest-level features, "k_depth_quantize<int>", ... */
const char* lmx_ctx_device_kernel_name(lmx_ctx* ctx, int32_t kernel_id);
lmx_status lmx_ctx_set_profiling(lmx_ctx* ctx, int32_t enabled);
lmx_status lmx_ctx_kernel_time(lmx_ctx* ctx, int32_t kernel_id, double* total_ms, int64_t* launches);
lmx_status lmx_ctx_reset_profiling(lmx_ctx* ctx);
/* Algorithmic bytes one enqueue() of n_frames moves through kernel `kernel_id` (SURVEY.md 8d formula). */
lmx_status lmx_ctx_algorithmic_bytes(lmx_ctx* ctx, int32_t kernel_id, int32_t n_frames, double* bytes);

const char* lmx_last_error(void);
const char* lmx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LMX_H_ */
