/*
 * gsrast.h -- C ABI of libgsrast.so, the MI355X-native (gfx950) differentiable 3D-Gaussian rasterizer.
 *
 * This is the drop-in boundary for the reference's native layer
 *   $RAST = submodules/gaustudio-diff-gaussian-rasterization   (in GAP-LAB-CUHK-SZ/gaustudio)
 *   $RAST/cuda_rasterizer/rasterizer.h:20-92   class CudaRasterizer::Rasterizer { markVisible, forward, backward }
 * Each entry point below replaces one of those static methods: same argument meaning and order, plain
 * pointers and sizes, plus an explicit HIP stream (the reference launches on the legacy default stream).
 * The torch extension `_C` (gaustudio_amd/csrc/torch_binding.cpp) is a thin adapter over these, replacing
 * $RAST/rasterize_points.cu:35-231 / ext.cpp:15-19.
 *
 * Conventions shared with the reference:
 *   - all tensors float32, row-major, device memory of the current HIP device;
 *   - an absent optional input is a NULL pointer (forward.cu:205,241; backward.cu:406,410);
 *   - viewmatrix / projmatrix are float[16] holding the column-major 4x4 (i.e. the transposed
 *     torch tensors gaustudio's Camera builds, datasets/__init__.py:154-159);
 *   - outputs are CHW planes (forward.cu:387-395).
 * Differences, all deliberate:
 *   - `background`, `viewmatrix`, `projmatrix`, `cam_pos` may live in HOST or DEVICE memory
 *     (gaustudio's renderers pass a CPU `bg`, renderers/vanilla_renderer.py:23);
 *   - the three opaque buffers are obtained through C callbacks instead of std::function
 *     (rasterizer.h:38-40); their internal layout is private to this library;
 *   - gsr_backward takes uninitialised OUTPUT pointers plus one scratch buffer; the reference wanted
 *     ten pre-zeroed tensors of which two (dL_dconic, dL_ddepth) were scratch (rasterize_points.cu:160-169);
 *   - errors are return codes + gsr_last_error() instead of C++ exceptions.
 */
#ifndef GSRAST_H_INCLUDED
#define GSRAST_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_ERR_HIP (-1)         /* a HIP runtime call or kernel failed; see gsr_last_error() */
#define GSR_ERR_ARG (-2)         /* invalid argument (e.g. neither SH nor colours; rasterizer_impl.cu:245-248) */
#define GSR_ERR_PREFILTERED (-3) /* a point was culled although `prefiltered` is set (auxiliary.h:156-160) */
#define GSR_ERR_ALLOC (-4)       /* an allocator callback returned NULL */
#define GSR_ERR_NONFINITE (-5)   /* gsr_knn, gsr_fusion_smooth, gsr_outlier_*: a point coordinate is not finite */
#define GSR_ERR_NONFINITE_QUERY (-6) /* gsr_knn: a query coordinate is not finite */

/* Replaces std::function<char*(size_t)> (rasterizer.h:38-40): must return device memory of at
 * least `bytes` bytes, 256-byte aligned, that stays valid until the matching backward has run.
 * gsr_forward may call the BINNING allocator twice (first with its remembered capacity, then -- only if that turned
 * out too small -- with the exact size; the second result replaces the first, which may be released in stream
 * order, as torch's resize_ does). */
typedef char* (*gsr_alloc_fn)(void* ctx, size_t bytes);

/* ABI version of this header (bumped on any signature change). */
int gsr_abi_version(void);

/* Message of the last error on the calling thread ("" if none). */
const char* gsr_last_error(void);

/* Replaces Rasterizer::markVisible (rasterizer.h:24-29; rasterizer_impl.cu:141-153).
 * present[i] = 1 iff Gaussian i passes the near-plane test p_view.z > 0.2 (auxiliary.h:154). */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     unsigned char* present, void* stream);

/* Replaces Rasterizer::forward (rasterizer.h:31-59; rasterizer_impl.cu:198-343).
 * Returns num_rendered (>= 0) or a negative GSR_ERR_*.  num_rendered keeps the reference's definition -- the sum
 * over visible Gaussians of the tiles of their getRect square (rasterizer_impl.cu:280-284) -- although fewer
 * instances are actually binned (only tiles that can hold a pixel with alpha >= 1/255; gsr_inspect_counts).
 * D = active SH degree, M = SH coefficients per Gaussian as stored (row stride of `shs`).
 * Exactly one of {shs, colors_precomp} and one of {scales+rotations, cov3D_precomp} must be non-NULL.
 * out_color[3,H,W], out_depth[1,H,W], out_median_depth[3,H,W], out_opacity[1,H,W], radii[P] are
 * fully overwritten (no pre-zeroing needed).  The host waits once for num_rendered (the reference blocks the
 * device as well, rasterizer_impl.cu:283-284); here the remaining kernels are already enqueued by then. */
int gsr_forward(gsr_alloc_fn geometry_alloc, void* geometry_ctx,
                gsr_alloc_fn binning_alloc, void* binning_ctx,
                gsr_alloc_fn image_alloc, void* image_ctx,
                int P, int D, int M,
                const float* background,
                int width, int height,
                const float* means3D,
                const float* shs,
                const float* colors_precomp,
                const float* opacities,
                const float* scales,
                float scale_modifier,
                const float* rotations,
                const float* cov3D_precomp,
                const float* viewmatrix,
                const float* projmatrix,
                const float* cam_pos,
                float tan_fovx, float tan_fovy,
                int prefiltered,
                float* out_color,
                float* out_depth,
                float* out_median_depth,
                float* out_opacity,
                int* radii,
                int debug,
                void* stream);

/* Bytes of device scratch gsr_backward needs for P Gaussians and R = num_rendered instances
 * (49 B per instance: the per-instance partial-gradient rows that replace the reference's float
 * atomics, backward.cu:559-607, plus one validity byte each; the per-Gaussian row offsets live in the
 * geometry buffer). */
size_t gsr_backward_scratch_bytes(int P, int R);

/* Lower bounds on the sizes of the geometry / image buffers a gsr_forward with these dimensions requests
 * (adapters use them to reject buffers that cannot belong to the backward they are handed to). */
size_t gsr_geometry_bytes(int P);
size_t gsr_image_bytes(int width, int height);

/* Replaces Rasterizer::backward (rasterizer.h:61-91; rasterizer_impl.cu:347-452).
 * R = num_rendered returned by the matching gsr_forward; geom/binning/image buffers are the ones its
 * allocators returned, unmodified and in full (besides the sorted lists the binning buffer carries the forward's
 * 16-bit block mask of every list entry, which the compositing backward reads instead of recomputing a cull; a
 * flag in the image buffer says whether the forward left them).  Outputs (all fully overwritten, rows of culled Gaussians = 0):
 *   dL_dmean2D[P,3] (xy used, already scaled by 0.5*W / 0.5*H, backward.cu:493-494,598-599),
 *   dL_dopacity[P], dL_dcolor[P,3], dL_dmean3D[P,3], dL_dcov3D[P,6] (may be NULL when cov3D_precomp is NULL: the gradient
 *   of a covariance the operator built itself from scale / rotation has no reader), dL_dsh[P,M,3] (may be NULL if M==0),
 *   dL_dscale[P,3], dL_drot[P,4].
 * Only channel 0 of dL_dpix_median_depth[3,H,W] is read (backward.cu:481-482).
 * Each of dL_dpix[3,H,W], dL_dpix_depth[1,H,W], dL_dpix_median_depth, dL_dpix_final_opacity[1,H,W] may be NULL: the loss does not
 * use that output, its gradient is zero -- nothing is loaded for it and no zero plane has to be materialised by the caller (the
 * reference reads all four, backward.cu:476-483, so its binding fills zeros); results are bit-equal to a call with explicit zero
 * planes.  Colour alone (the other three NULL: the usual 3DGS training loss) runs a compositing kernel specialised on it. */
int gsr_backward(int P, int D, int M, int R,
                 const float* background,
                 int width, int height,
                 const float* means3D,
                 const float* shs,
                 const float* colors_precomp,
                 const float* scales,
                 float scale_modifier,
                 const float* rotations,
                 const float* cov3D_precomp,
                 const float* viewmatrix,
                 const float* projmatrix,
                 const float* campos,
                 float tan_fovx, float tan_fovy,
                 const int* radii,
                 const char* geom_buffer,
                 const char* binning_buffer,
                 const char* image_buffer,
                 const float* dL_dpix,
                 const float* dL_dpix_depth,
                 const float* dL_dpix_median_depth,
                 const float* dL_dpix_final_opacity,
                 float* dL_dmean2D,
                 float* dL_dopacity,
                 float* dL_dcolor,
                 float* dL_dmean3D,
                 float* dL_dcov3D,
                 float* dL_dsh,
                 float* dL_dscale,
                 float* dL_drot,
                 char* scratch,
                 int debug,
                 void* stream);

/* gsr_backward in stages (new; lets the caller overlap a collective with the tail of the backward,
 * gaustudio_amd/parallel.py): `parts` selects GSR_BWD_PART_MAIN (compositing backward + the per-Gaussian geometry
 * stage: every output except dL_dsh, and dL_dmean3D still lacks its SH term) and / or GSR_BWD_PART_SH (the SH
 * stage for the Gaussians [sh_g0, sh_g1), sh_g0 a multiple of 256: writes those rows of dL_dsh and adds their SH
 * term to dL_dmean3D; needs MAIN to have run on the same buffers).  gsr_backward == both parts over [0, P). */
#define GSR_BWD_PART_MAIN 1
#define GSR_BWD_PART_SH 2
/* with GSR_BWD_PART_SH (gsr_backward_ex only): the SH stage in its FACTORED form for the multi-GPU gradient exchange
 * (gaustudio_amd/parallel.py FactoredGradExchange) -- dL_dsh is not written (may be NULL); dL_dcolor[P,3] is overwritten
 * in place with dRGB, the clamp-masked colour gradient the SH basis is multiplied with (backward.cu:35-40); dL_dmean3D
 * gets its SH term as usual.  SH colours in one [P,M,3] tensor only. */
#define GSR_BWD_PART_SH_COLORS 4
/* with GSR_BWD_PART_SH_COLORS, on every call of one backward (gsr_backward_ex only): the GEOMETRY stage of GSR_BWD_PART_MAIN
 * already leaves dRGB in dL_dcolor (the clamp mask is in the forward's record: it needs no SH coefficients), and the SH stage
 * does not write dL_dcolor again.  A caller that runs MAIN and SH as two calls can start the all-gather of this view's colour
 * gradients between them -- before the SH-direction stage has read 192 B of coefficients per Gaussian -- without a race on
 * the slot.  Same bits as the one-call form. */
#define GSR_BWD_PART_COLORS_EARLY 8
/* BANDED backward (round 6, gsr_backward_ex only; gaustudio_amd/parallel.py FactoredGradExchange(bands=2)): the compositing backward
 * and the per-Gaussian geometry stage of GSR_BWD_PART_MAIN run as TWO calls on the same buffers and the same scratch, so that a
 * caller can start exchanging the finished part of the gradients while the other half of the image is still composited:
 *   parts = MAIN | GSR_BWD_PART_BAND_FIRST  [| SH_COLORS | COLORS_EARLY], sh_g0 = split tile row S (0 <= S <= tile rows):
 *       composites the tile rows [0, S) and writes every output row except dL_dsh of the Gaussians of CLASS 1 = those that are
 *       invisible (radii == 0: zeros) or whose tile rect ends at or before row S -- all of their per-instance rows exist now;
 *   parts = MAIN | GSR_BWD_PART_BAND_SECOND [| ...], sh_g0 = the same S: composites the rows [S, tile rows) and writes the
 *       Gaussians of CLASS 2 (the others).
 * Together the two calls write every Gaussian exactly once, each from exactly the rows, in exactly the order, of the one-call
 * backward: BIT-IDENTICAL outputs.  No SH part in a band call (it follows the second band: GSR_BWD_PART_SH over [0, P));
 * gsr_band_classes tells the classes apart.  (With a forward that itself rendered a tile band, S counts tile rows of the
 * whole image as the forward's tile_row_lo / tile_row_hi do.) */
#define GSR_BWD_PART_BAND_FIRST 16
#define GSR_BWD_PART_BAND_SECOND 32
/* first[g] = 1 if Gaussian g is visible and of class 1 for split row S (its gradient rows are final after the FIRST band call),
 * second[g] = 1 if visible and of class 2; 0 otherwise (int32[P] each, device memory; either may be NULL).  Fed to
 * gsr_visible_index they give the headers of the two packed colour messages of a banded view. */
int gsr_band_classes(int P, const int* radii, const char* geom_buffer, int split_tile_row, int* first, int* second, void* stream);
int gsr_backward_parts(int parts, int sh_g0, int sh_g1, int P, int D, int M, int R, const float* background, int width,
                       int height, const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp, float tan_fovx,
                       float tan_fovy, const int* radii, const char* geom_buffer, const char* binning_buffer,
                       const char* image_buffer, const float* dL_dpix, const float* dL_dpix_depth,
                       const float* dL_dpix_median_depth, const float* dL_dpix_final_opacity, float* dL_dmean2D,
                       float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                       float* dL_dscale, float* dL_drot, char* scratch, int debug, void* stream);

/* The other half of the factored exchange: dL_dsh[P,M,3] = sum over the N views r = 0 .. N-1, in this order, of
 * basis_D(normalize(means3D[g] - campos[r])) (x) colors[r][g], i.e. the SH gradient of a multi-view step rebuilt from
 * the per-view dRGB (what GSR_BWD_PART_SH_COLORS leaves in dL_dcolor; rows of Gaussians culled in a view are zero there)
 * and the views' camera centres campos[N,3] (device memory).  Same arithmetic as the per-view SH backward and a fixed
 * order of views: bit-identical to accumulating the N per-view gradients one after the other.  colors[N,P,3].
 * (new; the reference has no multi-GPU path at all) */
int gsr_sh_grad_from_colors(int P, int D, int M, int N, const float* means3D, const float* campos, const float* colors,
                            float* dL_dsh, void* stream);

/* ---- compacted rows for the multi-GPU exchange (new; gaustudio_amd/parallel.py FactoredGradExchange(compact="view")) ----
 * A view of a real capture sees a fraction of the scene and the gradient rows of a Gaussian culled in a view are exactly zero,
 * so a view's colour gradients travel as a MESSAGE of 32-bit words:
 *   [0] K = visible Gaussians (radii > 0), [1] P, [2..3] 0; ceil(P/256) block bases (visible Gaussians in front of each
 *   256-Gaussian block); ceil(P/32) mask words (bit g & 31 of word g >> 5); padding to gsr_msg_header_words(P); then K rows.
 * gsr_visible_index builds the header from `radii` (right after the forward, off the critical path; scratch_counts:
 * ceil(P/256) words of device scratch), gsr_union_index the header of the OR of N messages' masks (message r starts at word
 * msg_offsets[r] of msgs; offsets in device memory); gsr_pack_rows copies the rows in[P,C] of the header's Gaussians to out[row * out_stride + col0 ..], gsr_unpack_rows
 * the other way (rows of other Gaussians are left untouched); gsr_sh_grad_from_packed is gsr_sh_grad_from_colors reading N
 * messages (rows of 3 floats behind each header) instead of dense [N,P,3] colours: same arithmetic, same order, same bits. */
size_t gsr_msg_header_words(int P);
int gsr_visible_index(int P, const int* radii, uint32_t* msg, uint32_t* scratch_counts, void* stream);
int gsr_union_index(int P, int N, const uint32_t* msgs, const unsigned long long* msg_offsets, uint32_t* out_hdr, uint32_t* scratch_counts,
                    void* stream);
int gsr_pack_rows(int P, int C, const uint32_t* hdr, const float* in, float* out, int out_stride, int col0, void* stream);
int gsr_unpack_rows(int P, int C, const uint32_t* hdr, const float* in, int in_stride, int col0, float* out, void* stream);
/* The geometry block of the exchange ([means3D 3 | opacity 1 | scales 3 | rotations 4] = 11 floats per Gaussian, four tensors) in one
 * pass each way: gsr_pack_geometry writes rows[r * 11 ..] = the 11 floats of the r-th Gaussian of `hdr` (rows must hold hdr[0] rows)
 * and ORs 1 into *flag_outside (device word, cleared by the caller) when a Gaussian OUTSIDE the header has a non-zero value -- a
 * gradient the rasterizer cannot have produced (it writes zeros for culled Gaussians): the caller must then exchange the dense
 * block; gsr_unpack_geometry copies the rows back (other Gaussians untouched). */
int gsr_pack_geometry(int P, const uint32_t* hdr, const float* g_means3D, const float* g_opacity, const float* g_scales,
                      const float* g_rotations, float* rows, uint32_t* flag_outside, void* stream);
int gsr_unpack_geometry(int P, const uint32_t* hdr, const float* rows, float* g_means3D, float* g_opacity, float* g_scales,
                        float* g_rotations, void* stream);
int gsr_sh_grad_from_packed(int P, int D, int M, int N, const float* means3D, const float* campos, const uint32_t* msgs,
                            const unsigned long long* msg_offsets, float* dL_dsh, void* stream);

/* Process-wide tunables (also read from the environment at load: GSR_TIGHT_BINNING, GSR_CULL, GSR_FWD_VARIANT,
 * GSR_BWD_VARIANT, GSR_SPECULATIVE).  The first five never change a bit of the forward; they exist for A/B measurements
 * and parity tests:
 *   "tight_binning" 1|0  bin each Gaussian into the tight sub-rect of the reference's getRect square (default 1);
 *   "cull"          1|0  block-level culling + pcut pre-test in composite_fwd (default 1);
 *   "fwd_variant"   0 or -1 only: composite_fwd with per-quarter (4x4 pixel) instance lists.  1 named a per-wave (8x8) walk
 *                        that is no longer in the library: a gsr_forward* with it is GSR_ERR_ARG;
 *   "speculative"   1|0  enqueue binning + compositing before the host has read the instance count (default 1);
 *   "bwd_variant"   -1 = auto (gsr_selftest), bit 0 = keep the select on T in composite_bwd.  Bit 1 named the per-wave
 *                        (8x8) kernel that is no longer in the library: a gsr_backward* with it is GSR_ERR_ARG;
 *   "fast_exp"     0|1  process default of gsr_options.fast_exp (below);
 *   "tile_order"    1|0  (GSR_TILE_ORDER) backward of a SKEWED frame (longest tile list > 1024 entries and > 4x the mean): run
 *                        the tiles longest walk first instead of in XCD bands (two small extra launches; changes no result bit);
 *   "roctx"         0|1  (GSR_ROCTX) wrap every stage of gsr_forward / gsr_backward in a roctx range ("gsr.preprocess_fwd",
 *                        "gsr.scan", ... ) for rocprofv3 --marker-trace timelines; the marker library is dlopen()ed, get
 *                        returns 1 only if it was found;
 *   "forget_forwards" (set only) drop the host-side memory of which mode each live forward ran in: the next gsr_backward of such buffers
 *                        reads the forward's own 4-byte control word from the image buffer instead (tests; always correct, one small sync);
 *   "bin_capacity"  n    binning capacity (instances) assumed by the next gsr_forward on the current device
 *                        (0 = forget; tests use a small n to force the re-allocate-and-relaunch path);
 *   "tile_row_lo", "tile_row_hi"  tile-grid sharding of ONE view across processes: only the 16-pixel
 *                        tile rows [lo, hi) are binned, composited and differentiated; pixels outside the band come
 *                        back as an empty scene's, gradients are the band's partial sums (SUM them over the ranks);
 *                        radii and num_rendered keep describing the whole view.  hi <= 0: the whole image. */
int gsr_set_option(const char* name, int value);
int gsr_get_option(const char* name);

/* ---- per-call options (ABI v6).  The process-wide switches above change the behaviour of every caller in the
 * process; two configurations in one process (two tile bands from two threads, a bit-exact evaluation pass next to a
 * fast_exp training loop) need them per call.  Every field: -1 = take the process default (gsr_set_option /
 * environment).  gsr_forward_ex / gsr_backward_ex are the supersets of the plain and the raw entry points (an absent
 * input is NULL: `shs_rest` NULL = `shs` holds all M coefficients; activation_flags 0 = activated inputs) with the
 * options in front; opt == NULL = all defaults, and gsr_forward(...) == gsr_forward_ex(NULL, ...).
 * The backward of a forward must be given the same `fast_exp` (the adapters keep the options of the forward with the
 * graph; the forward also records what it ran with in the image buffer, and a debug-mode backward checks it).
 *   fast_exp  0|1   exp on the transcendental unit (v_exp_f32) in both compositing kernels instead of the reproducible
 *                   9-instruction polynomial: not bit-reproducible against the CPU oracle any more (values within
 *                   ~1e-6 relative, threshold flips attributed by tests/test_gpu_fastexp.py); default 0. */
typedef struct gsr_options {
	int32_t struct_bytes;   /* sizeof(gsr_options) of the caller: fields beyond it are taken as -1 */
	int32_t tight_binning;
	int32_t cull;
	int32_t fwd_variant;
	int32_t bwd_variant;
	int32_t speculative;
	int32_t tile_row_lo;    /* tile band of THIS call: [lo, hi), hi <= 0 with lo >= 0 = the whole image */
	int32_t tile_row_hi;
	int32_t fast_exp;
	int32_t forward_only;   /* 0|1  (default 0) this forward will have no backward: skip what only a backward reads (the 36 B per Gaussian
	                         * of d(rgb)/d(view direction) that preprocess_fwd leaves for the SH backward).  gsr_backward on the buffers of
	                         * such a forward (any `parts`) is refused: from a host-side memory of the last 64 forwards, and -- debug = 1 --
	                         * from the forward's own record in the image buffer.  The Python adapters set it for calls under
	                         * torch.no_grad() (the grad mode is captured by the module wrapper: ctx.needs_input_grad ignores it) and for
	                         * calls none of whose inputs requires a gradient. */
} gsr_options;
void gsr_options_init(gsr_options* opt);   /* struct_bytes = sizeof, every field -1 */

int gsr_forward_ex(const gsr_options* opt, gsr_alloc_fn geometry_alloc, void* geometry_ctx, gsr_alloc_fn binning_alloc,
                   void* binning_ctx, gsr_alloc_fn image_alloc, void* image_ctx, int P, int D, int M,
                   const float* background, int width, int height, const float* means3D, const float* shs,
                   const float* shs_rest, const float* colors_precomp, const float* opacities, const float* scales,
                   float scale_modifier, const float* rotations, const float* cov3D_precomp, int activation_flags,
                   const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                   int prefiltered, float* out_color, float* out_depth, float* out_median_depth, float* out_opacity,
                   int* radii, int debug, void* stream);
/* parts / sh_g0 / sh_g1 as in gsr_backward_parts; dL_dsh_rest NULL unless shs_rest is given. */
int gsr_backward_ex(const gsr_options* opt, int parts, int sh_g0, int sh_g1, int P, int D, int M, int R,
                    const float* background, int width, int height, const float* means3D, const float* shs,
                    const float* shs_rest, const float* colors_precomp, const float* scales, float scale_modifier,
                    const float* rotations, const float* cov3D_precomp, int activation_flags, float tan_fovx,
                    float tan_fovy, const int* radii, const char* geom_buffer, const char* binning_buffer,
                    const char* image_buffer, const float* dL_dpix, const float* dL_dpix_depth,
                    const float* dL_dpix_median_depth, const float* dL_dpix_final_opacity, float* dL_dmean2D,
                    float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                    float* dL_dsh_rest, float* dL_dscale, float* dL_drot, char* scratch, int debug, void* stream);

/* Device self-test of the arithmetic identities composite_bwd relies on: bit 0: v_rcp_f32(1.0) == 1.0,
 * bit 1: t * v_rcp_f32(1.0) == t.  Synchronises the stream.  Negative = GSR_ERR_*. */
int gsr_selftest(void* stream);

/* ---- fused parameter activations (new, not in the reference's interface) ----
 * gsr_forward_raw / gsr_backward_raw take GauStudio's RAW point-cloud attributes -- f_dc[P,1,3] and f_rest[P,M-1,3]
 * instead of the concatenated sh[P,M,3] (models/vanilla_sg.py:103-106), pre-activation opacity / scale / rotation --
 * and apply VanillaPointCloud's activations inside the kernels (models/vanilla_sg.py:33-37: exp, sigmoid,
 * F.normalize) according to activation_flags.  Gradients are returned w.r.t. the raw attributes. */
#define GSR_ACT_OPACITY_SIGMOID 1
#define GSR_ACT_SCALE_EXP 2
#define GSR_ACT_ROT_NORMALIZE 4

int gsr_forward_raw(gsr_alloc_fn geometry_alloc, void* geometry_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                    gsr_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background, int width,
                    int height, const float* means3D, const float* f_dc, const float* f_rest, const float* raw_opacities,
                    const float* raw_scales, float scale_modifier, const float* raw_rotations, int activation_flags,
                    const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                    float tan_fovy, int prefiltered, float* out_color, float* out_depth, float* out_median_depth,
                    float* out_opacity, int* radii, int debug, void* stream);

int gsr_backward_raw(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                     const float* f_dc, const float* f_rest, const float* raw_scales, float scale_modifier,
                     const float* raw_rotations, int activation_flags, float tan_fovx, float tan_fovy,
                     const int* radii, const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                     const float* dL_dpix, const float* dL_dpix_depth, const float* dL_dpix_median_depth,
                     const float* dL_dpix_final_opacity, float* dL_dmean2D, float* dL_draw_opacity, float* dL_dcolor,
                     float* dL_dmean3D, float* dL_dcov3D, float* dL_df_dc, float* dL_df_rest, float* dL_draw_scale,
                     float* dL_draw_rot, char* scratch, int debug, void* stream);

/* ---- introspection of the opaque buffers (tests, debugging).  The reference exposes the same state
 * only implicitly through GeometryState/BinningState/ImageState (rasterizer_impl.h:33-64).
 * Any output pointer may be NULL.  All outputs are device memory. ---- */

/* means2D[P,2], depths[P], conic_opacity[P,4], rgb[P,3], clamped[P,3] (0/1 bytes), tiles_touched[P].
 * Rows of culled Gaussians (radii==0) are written as zeros. */
int gsr_inspect_geometry(const char* geom_buffer, int P, const int* radii, float* means2D, float* depths,
                         float* conic_opacity, float* rgb, unsigned char* clamped,
                         uint32_t* tiles_touched, void* stream);

/* After gsr_backward: sums[P,10] = the per-Gaussian totals of the compositing stage that feed the
 * per-Gaussian stage, in the order {dL_dmean2D.x, .y, dL_dconic a, b, c, dL_dopacity, dL_dcolor r, g, b,
 * dL_ddepth} (what the reference accumulates with atomicAdd, backward.cu:559-607), recomputed from
 * the scratch rows with the same fixed summation order gsr_backward used. */
int gsr_inspect_backward_sums(const char* geom_buffer, const char* scratch, int P, int R, const int* radii,
                               float* sums, void* stream);

/* out = { instances binned (tight rects; the length of point_list), longest tile list, the reference-defined
 * num_rendered (what gsr_forward returned), error flags: bit 0 = the reference-defined count overflowed 2^31 - 1, bit 1 = the
 * long-list sort overflowed one of its work queues (a capacity bound violated: point_list is not completely sorted; debug-mode
 * gsr_forward / gsr_backward calls fail on it) }.  `out` is HOST memory; synchronises the stream. */
int gsr_inspect_counts(const char* image_buffer, int width, int height, uint32_t out[4], void* stream);

/* Instances composite_fwd actually STAGED for this frame, summed over the tiles: a tile's workgroup stops fetching its list once
 * every pixel of the tile has saturated (forward.cu:278-285 `done`), 256 entries at a time -- on dense frames (C4: lists of 3.4 k
 * entries, 99 % of the pixels saturate after a few hundred) that is a fraction of the binned instances, and it is the count the
 * kernel's byte traffic follows (bench.py's `roofline`).  Left by the kernel in the image buffer's (by then dead) tile counters.
 * `staged_total` is HOST memory; synchronises the stream.  Valid after a gsr_forward with P > 0 and at least one instance. */
int gsr_inspect_staged(const char* image_buffer, int width, int height, unsigned long long* staged_total, void* stream);

/* point_list[R] (Gaussian ids, tile-major, depth-sorted; R = instances binned, see gsr_inspect_counts),
 * ranges[T,2] ([start,end) per tile). */
int gsr_inspect_binning(const char* binning_buffer, const char* image_buffer, int R, int width, int height,
                        uint32_t* point_list, uint32_t* ranges, void* stream);

/* final_T[H,W], n_contrib[H,W] in pixel-major order (forward.cu:385-386). */
int gsr_inspect_image(const char* image_buffer, int width, int height, float* final_T,
                      uint32_t* n_contrib, void* stream);

/* ---- post-render epilogue: the step that follows the operator in gs-extract-mesh /
 * gs-extract-pcd.  `intrinsics` = 3x3 row-major K and `world_to_camera` = 4x4 row-major (Camera.extrinsics,
 * gaustudio/datasets/__init__.py:225-237) are HOST pointers (25 floats); depth / outputs are device memory. ---- */

/* Replaces Camera.depth2point(depth, 'camera' | 'world') (datasets/__init__.py:307-339 with ndc_2_cam :106-112):
 * points[H,W,3]; world_to_camera == NULL -> camera coordinates. */
int gsr_depth_to_points(const float* depth, int width, int height, const float* intrinsics,
                        const float* world_to_camera, float* points, void* stream);

/* Replaces Camera.depth2normal(depth, k, d_min, d_max, 'camera' | 'world') (datasets/__init__.py:342-380): five-tap
 * cross-product normals[H,W,3] of the unprojected depth, (-1,-1,-1) where any tap is outside (d_min, d_max) or
 * outside the image. */
int gsr_depth_to_normals(const float* depth, int width, int height, const float* intrinsics, int k, float d_min,
                         float d_max, const float* world_to_camera, float* normals, void* stream);
/* Both of the above in one pass, with the opacity mask of gs-extract-mesh in front (extract_mesh.py:104-110: the depth of a
 * pixel with opacity < min_opacity counts as 0, so its point is the camera centre and its normal invalid): depth[H,W],
 * opacity[H,W] or NULL (no mask), points[H,W,3] and normals[H,W,3] in the coordinates world_to_camera selects (NULL =
 * camera), either output may be NULL.  Tap distance (k - 1) / 2 <= 2.  Same arithmetic per value as the separate calls. */
int gsr_depth_epilogue(const float* depth, const float* opacity, float min_opacity, int width, int height,
                       const float* intrinsics, int k, float d_min, float d_max, const float* world_to_camera, float* points,
                       float* normals, void* stream);

/* Replaces masked_bilateral_filter (gaustudio/scripts/extract_pcd.py:185-238: numpy + cv2.dilate + cv2.bilateralFilter
 * on the CPU, between the render and depth2point in gs-extract-pcd).  mask[H,W] u8 (non-zero = valid) -> new_mask[H,W]
 * u8 (valid iff the whole d x d window is valid), filtered[H,W]: the bilateral filter (OpenCV's float32 definition:
 * radius max(d/2,1), circular window, reflect-101 border) of the depth normalised over new_mask with everything else
 * set to 0, de-normalised; pixels outside new_mask keep their input depth.  d odd (or 0 = from sigma_space);
 * scratch2 = 8 bytes of device memory.
 * Border: cv2's BORDER_REFLECT_101, reflected until the index is inside (|p| mod 2(n - 1), folded; a single row or column
 * gives index 0), so an image narrower than the radius is crossed more than once.
 * NaN: a NaN depth inside new_mask is outside the valid region, as with the reference's nanmin / nanmax: it does not enter
 * the min / max, is 0 in the normalised image and comes back as NaN; new_mask does not depend on the depth values.
 * d = 0: radius = lrint(1.5 sigma_space) (at least 1) and the erosion window is 2 radius + 1.  That window is this
 * library's own choice: the reference only ever passes d = 3 (cv2.dilate with a 0 x 0 kernel has no meaning to follow).
 * sigma <= 0 counts as 1.  Parity with cv2 is unpinned (the library is not in this image): restated
 * from its published algorithm, colour weight by expf instead of cv2's 4096-bin interpolated table. */
int gsr_masked_bilateral(const float* depth, const unsigned char* mask, int width, int height, int d, float sigma_color,
                         float sigma_space, float* filtered, unsigned char* new_mask, unsigned int* scratch2, void* stream);

/* ---- TSDF fusion + iso-surface extraction: what gs-extract-mesh does with the rendered
 * depth points (gaustudio/scripts/extract_mesh.py:86,115,145 -> vdbfusion.VDBVolume.integrate /
 * .extract_triangle_mesh, a CPU library the reference pip-installs).  Stateless: the volume is caller-owned device
 * memory --
 *   block_keys[capacity] u64, all bits set = empty (capacity a power of two; 8x8x8-voxel blocks, open addressing);
 *   voxels[capacity * 512] u64, zero-initialised: (sum_q << 24) | count with sum_q the sum of tsdf / sdf_trunc in
 *       2^-15 fixed point (a block's voxels live at its hash slot; the fields hold up to 2^24 - 1 observations
 *       of a voxel);
 *   status[1] u32, zero-initialised: bit 0 set when the hash table overflowed (the ray that hit it is dropped from there
 *       on), bit 1 when a voxel was offered more than 2^24 - 2^20 = 15 728 640 observations (the surplus is dropped; the
 *       count is declared full 2^20 below the field's capacity so that the overflow guard needs no second atomic).
 * Algorithm and parity status: gaustudio_amd/csrc/gsr_tsdf.hip, DESIGN.md s8. ---- */

/* VDBVolume::Integrate(points, origin) with the default weighting (weight 1): points[num_points,3] device,
 * origin[3] host.  Points within 1e-3 voxels of the origin (and non-finite ones) are skipped: that is what depth2point
 * makes of a masked pixel (depth 0), so a whole point map can be passed without compacting the valid pixels. */
int gsr_tsdf_integrate(const float* points, int num_points, const float origin[3], float voxel_size, float sdf_trunc,
                       int space_carving, uint64_t* block_keys, uint64_t capacity, uint64_t* voxels, uint32_t* status,
                       void* stream);
/* The same for an image-shaped point map [num_points / row_width][row_width] (what gsr_depth_to_points returns for a
 * frame; row_width must divide num_points, 0 = plain list): workgroups take 32 x 32 patches of the map, whose rays share
 * voxels in both image directions, and commit several times fewer atomics (2.3x faster at 1080p).  The volume is bit-identical to gsr_tsdf_integrate's. */
int gsr_tsdf_integrate_map(const float* points, int num_points, int row_width, const float origin[3], float voxel_size,
                           float sdf_trunc, int space_carving, uint64_t* block_keys, uint64_t capacity, uint64_t* voxels,
                           uint32_t* status, void* stream);

/* Test / inspection: for the listed hash slots, per voxel (x fastest) the observation count, the mean tsdf
 * (+sdf_trunc where the count is 0) and the raw fixed-point sum. */
int gsr_tsdf_export_blocks(const uint64_t* voxels, const uint32_t* block_slots, int num_blocks, float sdf_trunc,
                           uint32_t* counts, float* tsdf, int64_t* sums, void* stream);

/* VDBVolume::ExtractTriangleMesh(fill_holes, min_weight) in two steps around a caller-side exclusive scan.
 * block_slots[num_blocks]: the occupied hash slots in the order the mesh should be emitted; slot_to_block[capacity]:
 * its inverse.  classify writes cases[num_blocks*512] (u8), edge_flags[num_blocks*512] (u32) and the per-block
 * vertex / triangle counts; emit takes their exclusive scans and writes vertices[nv,3] (f32, world units),
 * triangles[nt,3] (i32, outward winding: normals point towards positive tsdf) and vertex_base[num_blocks*512]. */
int gsr_tsdf_mc_classify(const uint64_t* block_keys, uint64_t capacity, const uint64_t* voxels, const uint32_t* block_slots,
                         int num_blocks, const uint32_t* slot_to_block, float sdf_trunc, float min_weight, int fill_holes,
                         uint8_t* cases, uint32_t* edge_flags, uint32_t* block_num_vertices, uint32_t* block_num_triangles,
                         void* stream);
int gsr_tsdf_mc_emit(const uint64_t* block_keys, uint64_t capacity, const uint64_t* voxels, const uint32_t* block_slots,
                     int num_blocks, const uint32_t* slot_to_block, float voxel_size, float sdf_trunc, const uint8_t* cases,
                     const uint32_t* edge_flags, const uint32_t* block_vertex_offset, const uint32_t* block_triangle_offset,
                     uint32_t* vertex_base, float* vertices, int* triangles, void* stream);

/* ---- Coloured TSDF from posed RGB-D frames: what the `tsdf` initializer does on the CPU
 * (gaustudio/pipelines/initializers/mesh.py:445-514 -> Open3D ScalableTSDFVolume(color_type=RGB8).integrate /
 * .extract_triangle_mesh).  Additive to ABI 6.  Voxel-projective: every voxel of every block a frame's depth touches projects
 * into the depth image and keeps float running averages.  Stateless; the volume is caller-owned device memory --
 *   block_keys[capacity] u64 and status[1] u32 exactly as above (bit 0: the hash overflowed);
 *   voxels[capacity * 5 * 512] f32, zero-initialised: per hash slot the planes tsdf (in units of sdf_trunc), weight, r, g, b
 *       (0..255) of the block's 512 voxels, x fastest;
 *   slot_stamp[capacity] i32, zero-initialised: the number of the last frame that touched the slot.
 * Voxel (i,j,k) has its centre at ((i,j,k) + 0.5) voxel_length.  Matrices are rows 0..2 of a rigid 4x4, row-major, HOST.
 * Semantics, operation by operation: tests/tsdf_rgbd_model.py; contract: INTEGRATION.md s18; design: DESIGN.md s15. ---- */

/* Allocation: for every pixel (u, v) with u % stride == 0 and v % stride == 0 whose cleaned depth d (non-finite, negative
 * and > depth_trunc count as 0) is > 0, opens every block that intersects the box +-sdf_trunc around
 * cam_to_world ((u - cx) d / fx, (v - cy) d / fy, d) and stores `frame` (> 0) into slot_stamp of its slot.  intrinsic = {fx, fy,
 * cx, cy}.  lane_filter != 0: a lane whose box of blocks equals its lane-neighbour's leaves the insertion to it (same
 * result, fewer hash probes); counters (device, optional) [0] += insertions asked for, [1] += insertions made. */
int gsr_ctsdf_touch(const float* depth, int width, int height, int stride, const float intrinsic[4], const float cam_to_world[12],
                    float depth_trunc, float voxel_length, float sdf_trunc, uint64_t* block_keys, uint64_t capacity,
                    int* slot_stamp, int frame, uint32_t* status, int lane_filter, uint64_t* counters, void* stream);
/* Integration of one frame into the listed slots (those stamped by gsr_ctsdf_touch for this frame, any order, no slot twice).
 * color_mode 0: u8 [H,W,3]; 1: f32 [H,W,3] in [0,1]; 2: f32 [3,H,W] in [0,1] (float colour is quantised on load:
 * uint8(clip(x * 255, 0, 255)), truncating).  No atomics: one thread owns one voxel. */
int gsr_ctsdf_integrate(const float* depth, const void* color, int color_mode, int width, int height, const float intrinsic[4],
                        const float world_to_cam[12], float depth_trunc, float voxel_length, float sdf_trunc,
                        const uint64_t* block_keys, const int* touched_slots, int num_touched, float* voxels, void* stream);
/* Test / inspection: tsdf[n*512], weight[n*512], color[n*512*3] of the listed slots (x fastest). */
int gsr_ctsdf_export_blocks(const float* voxels, const uint32_t* block_slots, int num_blocks, float* tsdf, float* weight, float* color,
                            void* stream);
/* ExtractTriangleMesh in the two steps of gsr_tsdf_mc_classify / _emit (same block lists, scans, tables and vertex sharing).
 * A cube is meshed iff all 8 corner voxels have weight > 0 and weight >= min_weight; inside = tsdf < 0.  emit also writes
 * colors[nv,3] f32 in [0,1]: the linear interpolation of the edge's two voxel colours at the zero crossing. */
int gsr_ctsdf_mc_classify(const uint64_t* block_keys, uint64_t capacity, const float* voxels, const uint32_t* block_slots, int num_blocks,
                          const uint32_t* slot_to_block, float min_weight, uint8_t* cases, uint32_t* edge_flags,
                          uint32_t* block_num_vertices, uint32_t* block_num_triangles, void* stream);
int gsr_ctsdf_mc_emit(const uint64_t* block_keys, uint64_t capacity, const float* voxels, const uint32_t* block_slots, int num_blocks,
                      const uint32_t* slot_to_block, float voxel_length, const uint8_t* cases, const uint32_t* edge_flags,
                      const uint32_t* block_vertex_offset, const uint32_t* block_triangle_offset, uint32_t* vertex_base, float* vertices,
                      float* colors, int* triangles, void* stream);

/* ---- 2D Gaussian surfels ("2DGS": the operator behind diff_surfel_rasterization) ----
 * Additive to ABI 6.  The same allocator callbacks, stream and gsr_options as gsr_forward_ex (fast_exp is honoured; the binning
 * options do not apply: surfels are binned into the reference's square tile rects).  scales are [P,2], rotations [P,4]
 * (normalised inside), exactly one of shs [P,M,3] / colors_precomp [P,3].  Outputs: out_color [3,H,W] (composited colour + T bg),
 * out_allmap [7,H,W] = {expected depth, alpha, normal xyz (view space), median depth, depth distortion}, radii [P].
 * Returns the number of (tile, surfel) instances R (>= 0) or a negative GSR_ERR_*.  The forward reads R back before it sizes
 * the binning buffer (one host wait per call).  Semantics and constants: INTEGRATION.md "2D Gaussian surfels". */
int gsr_surfel_forward(const gsr_options* opt, gsr_alloc_fn geometry_alloc, void* geometry_ctx, gsr_alloc_fn binning_alloc,
                       void* binning_ctx, gsr_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background,
                       int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                       const float* viewmatrix, const float* projmatrix, const float* cam_pos, float* out_color, float* out_allmap,
                       int* radii, int debug, void* stream);
/* bytes of the `scratch` a gsr_surfel_backward of R instances needs (one 64-B row of partial sums per instance) */
size_t gsr_surfel_scratch_bytes(int P, int R);
/* Backward of gsr_surfel_forward: the three buffers it filled, its outputs out_color / out_allmap (the compositing backward walks
 * front to back and needs the totals) and the upstream gradients dL_dout_color [3,H,W] / dL_dout_allmap [7,H,W] (NULL = zero).
 * Writes dL_dmean2D [P,3] (the 2DGS densification proxy), dL_dopacity [P], dL_dcolor [P,3], dL_dmean3D [P,3], dL_dsh [P,M,3]
 * (only with shs), dL_dscale [P,2], dL_drot [P,4].  No float atomics: the result is bit-identical from run to run. */
int gsr_surfel_backward(const gsr_options* opt, int P, int D, int M, int R, int width, int height, const float* means3D,
                        const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                        const float* rotations, const int* radii, const char* geom_buffer, const char* binning_buffer,
                        const char* image_buffer, const float* out_color, const float* out_allmap, const float* dL_dout_color,
                        const float* dL_dout_allmap, float* dL_dmean2D, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                        float* dL_dsh, float* dL_dscale, float* dL_drot, char* scratch, int debug, void* stream);

/* ---- nearest neighbours, normal fusion and outlier removal: what gs-extract-pcd does after its render loop
 * (gaustudio/scripts/extract_pcd.py:108-183 normal_fusion, :30-51 clean_point_cloud; scipy cKDTree and Open3D on the CPU in
 * the reference).  Additive to ABI 6.  Stateless: inputs and outputs are caller-owned device memory, scratch comes from the
 * gsr_alloc_fn callback (called once or twice per call, device memory that must stay valid until the call's work on `stream`
 * has run), `stream` is the HIP stream of every launch.  Each entry reads a few values back to the host (the grid's cell
 * count, the number of fused ids), so it waits on `stream` once or more.  Returns GSR_OK (or a count, where stated) or
 * a negative GSR_ERR_*.  Algorithms, resources and parity status: gaustudio_amd/csrc/gsr_knn.hip, DESIGN.md s11,
 * INTEGRATION.md "gs-extract-pcd". ---- */
#define GSR_KNN_MAX_K 64

/* Exact k nearest neighbours: for each of queries[num_queries,3] (NULL = the points themselves; num_queries is then
 * ignored) the k nearest of points[num_points,3] (f32, all finite), 1 <= k <= min(64, num_points), in ascending
 * (squared distance, index) order: dist2[num_queries,k] (f64, computed from the f32 coordinates) and indices[num_queries,k]
 * (i64).  A query point that is also a data point finds itself first unless a duplicate with a lower index ties with it.
 * Every tie is broken by the index, so the output is fully determined.  num_queries = 0 with non-NULL queries writes nothing
 * (the grid is still built and the points are still checked).  GSR_ERR_ARG for a bad k or a NULL pointer,
 * GSR_ERR_NONFINITE for a point and GSR_ERR_NONFINITE_QUERY for a query coordinate that is NaN or infinite (the queries are
 * checked on the device while they are answered; dist2 and indices are then unspecified). */
int gsr_knn(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, const float* queries,
            int num_queries, int k, double* dist2, int64_t* indices, void* stream);

/* normal_fusion, per view (extract_pcd.py:118-126): for record i = (ids[i], normals[i,3], confidences[i]) of one view,
 * v = w2c_translation - xyz[ids[i]] (w2c_translation = extrinsics[:3,3] of the world-to-camera matrix, HOST float[3]) and
 * w = conf * |dot(v / |v|, n)| / (|v| + 1e-6) (fp64, stored f32).  Writes records[num_records,5] = {id, n.x, n.y, n.z, w}
 * (the id as int32, the rest as f32 bits).  An id outside [0, num_gaussians) sets bit 0 of status[1] (u32, caller-zeroed). */
int gsr_fusion_records(const float* xyz, int num_gaussians, const int* ids, const float* normals, const float* confidences,
                       int num_records, const float w2c_translation[3], int* records, int* status, void* stream);

/* normal_fusion, steps 1-3 (extract_pcd.py:109-168): groups records[num_records,5] by id (stable radix sort, so an id's
 * records are reduced in record order), and per id mean = normalize(sum n w / sum w) in fp64, then the same over the
 * records with |n - mean| < consistency (0/0 = NaN where none is consistent; kept).  Writes unique_ids[U] (ascending) and
 * mean_normals[U,3] (f32); both must hold min(num_records, num_gaussians) entries.  Returns U >= 0. */
int gsr_fusion_group(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* records, int num_records, int num_gaussians,
                     float consistency, int* unique_ids, float* mean_normals, void* stream);

/* normal_fusion, step 4 (extract_pcd.py:170-181): q = xyz[unique_ids]; per fused point its k nearest points of q (itself
 * included), s = sum_j mean_normals[nbr_j] * exp(-sqrt(d2_j) / sigma) in fp64, cast to f32, normals[U,3] = s / max(|s|,
 * 1e-12) in f32.  A NaN neighbour makes the point NaN.  GSR_ERR_ARG when num_unique < k. */
int gsr_fusion_smooth(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* xyz, const int* unique_ids,
                      const float* mean_normals, int num_unique, int k, float sigma, float* normals, void* stream);

/* Open3D PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio) as restated in INTEGRATION.md: a_i = mean of the
 * distances to the min(nb_neighbors, num_points) nearest points (itself included, at 0); mean and Bessel-corrected std over
 * the points with a_i > 0 (fixed-order fp64 reductions); keep[i] = 0 < a_i < mean + std_ratio * std (u8).
 * mean_distance[num_points] (f64, NULL = not wanted) receives a_i. */
int gsr_outlier_statistical(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points,
                            int nb_neighbors, double std_ratio, unsigned char* keep, double* mean_distance, void* stream);

/* remove_normal_outliers (extract_pcd.py:30-43): with the min(nb_neighbors, num_points) nearest points, neighbour 0 taken to
 * be the point itself and dropped, keep[i] = mean_j acos(|dot(n_j, n_i)|) < angle_threshold (fp64; a NaN mean drops the
 * point).  normals[num_points,3] f64. */
int gsr_outlier_normal(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, const double* normals,
                       int num_points, int nb_neighbors, double angle_threshold, unsigned char* keep, void* stream);

/* ---- triangle mesh rasterization: what gaustudio/scripts/render_mesh.py and texture_mesh.py take from PyTorch3D
 * (MeshRasterizer with blur_radius = 0, faces_per_pixel = 1: a hard z-buffer; interpolate_face_attributes;
 * Meshes.verts_normals_packed; get_visible_faces).  Additive to ABI 6, in the style of gsr_knn: inputs and outputs are
 * caller-owned device memory, scratch comes from the gsr_alloc_fn callback (called once or twice per call), `stream` is the
 * HIP stream of every launch; each entry reads a count or an error flag back, so it waits on `stream` once.  Forward only,
 * deterministic (no float atomics; bit-identical from run to run).  Contract: INTEGRATION.md s15; design: gsr_mesh.hip,
 * DESIGN.md s12. ---- */
#define GSR_MESH_MAX_CHANNELS 4

/* verts[num_verts,3] f32 world space, faces[num_faces,3] i32; intrinsics = 3x3 row-major K (fx, fy, cx, cy are read) and
 * extrinsics = 4x4 row-major world-to-camera matrix (OpenCV axes, Camera.extrinsics), both HOST pointers.  Pixel (i, j) casts
 * the camera-space ray ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1); each pixel keeps the hit with the least (z, face id),
 * a hit counting when z > z_near (z_near >= 0).  cull_backfaces != 0 keeps the faces with ((b - a) x (c - a)) . a < 0 in
 * camera space.  Outputs pix_to_face[H,W] i32, zbuf[H,W] f32 (camera z), bary[H,W,3] f32 (perspective-correct), -1 on
 * background.  Returns the number of (tile, face) entries binned (>= 0), or GSR_ERR_ARG for a face index outside
 * [0, num_verts), a non-positive or too large (> 16384) size, singular or non-finite intrinsics, a negative z_near. */
int gsr_mesh_rasterize(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                       int num_faces, const float intrinsics[9], const float extrinsics[16], int height, int width,
                       int cull_backfaces, float z_near, int* pix_to_face, float* zbuf, float* bary, void* stream);

/* interpolate_face_attributes for per-vertex attributes: out[p,c] = (b0 attr[f0,c] + b1 attr[f1,c]) + b2 attr[f2,c] with
 * (f0, f1, f2) = faces[pix_to_face[p]] and (b0, b1, b2) = bary[p]; 0 where pix_to_face[p] < 0.  attr[num_verts,channels],
 * 1 <= channels <= GSR_MESH_MAX_CHANNELS.  GSR_ERR_ARG when a face id >= num_faces or a face index is out of range. */
int gsr_mesh_interpolate(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* faces, int num_faces, const int* pix_to_face,
                         const float* bary, int num_pixels, const float* attr, int num_verts, int channels, float* out, void* stream);

/* Meshes.verts_normals_packed: corner k of face f adds (v[k+1] - v[k]) x (v[k+2] - v[k]) (indices mod 3) to its vertex, in
 * ascending (f, k) order in f32; normals[num_verts,3] = n / max(|n|, 1e-6).  GSR_ERR_ARG for a face index out of range. */
int gsr_mesh_vertex_normals(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                            int num_faces, float* normals, void* stream);

/* visible[num_faces] u8 = 1 for the faces that appear in pix_to_face[num_pixels], 0 elsewhere (texture_mesh.py
 * get_visible_faces as a mask).  GSR_ERR_ARG when a face id >= num_faces. */
int gsr_mesh_visible_faces(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* pix_to_face, int num_pixels, int num_faces,
                           unsigned char* visible, void* stream);

/* ---- mesh cleaning: the --clean stage of gaustudio/scripts/extract_mesh.py:149-186 (Open3D's cluster_connected_triangles,
 * the per-cluster areas, remove_triangles_by_mask + remove_unreferenced_vertices) for a mesh that stays in HBM.  Additive to
 * ABI 6, in the style of gsr_knn / gsr_mesh_*: inputs and outputs are caller-owned device memory, scratch comes from the
 * gsr_alloc_fn callback (called once per call), `stream` is the HIP stream of every launch; each entry reads counts and an
 * error flag back, so it waits on `stream` (gsr_mesh_cluster_triangles: once per batch of four rounds).  Deterministic: integer
 * atomics only, no float atomics; bit-identical from run to run.  Contract: INTEGRATION.md s16; design: gsr_mesh_clean.hip,
 * DESIGN.md s13. ---- */

/* faces[num_faces,3] i32 with indices in [0, num_verts), 3 num_faces < 2^31.  Two triangles are adjacent when they share an
 * undirected edge {min(a,b), max(a,b)} (a shared vertex alone does not connect; an edge with more than two triangles connects
 * all of them; a triangle that repeats an index behaves as its three literal edges say).  Writes triangle_clusters[num_faces]
 * (the cluster of each triangle) and cluster_n_triangles[C] (the buffer must hold num_faces entries); clusters are numbered in
 * ascending order of their lowest triangle index.  *rounds (HOST, may be NULL) receives the number of hook-and-jump rounds
 * run until one changed nothing (O(log num_faces), independent of the mesh's diameter).  Returns C >= 0, or GSR_ERR_ARG for a
 * face index outside [0, num_verts) (nothing is written then). */
int gsr_mesh_cluster_triangles(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* faces, int num_faces, int num_verts,
                               int* triangle_clusters, int* cluster_n_triangles, int* rounds, void* stream);

/* cluster_area[num_clusters] f64 = per cluster the sum of 0.5 |(v1 - v0) x (v2 - v0)| (fp64 from the f32 verts, Open3D
 * GetTriangleArea) over its triangles, in a fixed order: the triangles in ascending order in pieces of 1024, each piece summed
 * by 64 strided partial sums and a fixed tree, the pieces added in order.  GSR_ERR_ARG for a cluster index outside
 * [0, num_clusters) or a face index outside [0, num_verts). */
int gsr_mesh_cluster_area(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                          int num_faces, const int* triangle_clusters, int num_clusters, double* cluster_area, void* stream);

/* remove_triangles_by_mask + remove_unreferenced_vertices: the faces with keep[f] != 0 (u8) in their original order, the
 * vertices one of them references in their original order, the faces rewritten with the new vertex indices.  out_faces and
 * face_index (new face -> old face) must hold num_faces faces / entries, out_verts and vertex_index (new vertex -> old
 * vertex) num_verts; verts / out_verts may both be NULL (indices only).  Returns the number of kept faces and stores the
 * number of kept vertices in *num_verts_out (HOST); GSR_ERR_ARG for a face index outside [0, num_verts) (nothing is written). */
int gsr_mesh_compact(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                     int num_faces, const unsigned char* keep, float* out_verts, int* out_faces, int* vertex_index, int* face_index,
                     int* num_verts_out, void* stream);

/* ---- Shape-as-Points meshing: what gs-extract-pcd --meshing sap runs after the point cloud is cleaned
 * (gaustudio/models/sap.py, gaustudio/utils/graphics_utils.py:19-333: point_rasterize, the spectral solve of DPSR.forward,
 * grid_interp and its normalisation; a dense marching cubes in place of the CPU round trip through skimage).  Additive to
 * ABI 6, in the style of gsr_knn / gsr_mesh_*: inputs and outputs are caller-owned device memory, scratch comes from the
 * gsr_alloc_fn callback (called once per call), `stream` is the HIP stream of every launch; the entries that say so read a
 * flag or two counts back and wait on `stream` once.  The backward entries follow below.  Deterministic: no float atomics, bit-identical from run
 * to run.  Grids are dense, row-major [r0, r1, r2] f32 with every size >= 2 and r0 r1 r2 < 2^30.  The two FFTs between the
 * stages are the caller's.  Contract: INTEGRATION.md s17; design: gsr_psr.hip, DESIGN.md s14. ---- */
#define GSR_PSR_MAX_CHANNELS 4

/* point_rasterize (:157-217): points[num_points,3] f32 in [0, 1), values[num_points,channels] f32, 1 <= channels <= 4.
 * Per axis, in fp32: cubesize = 1 / size, ind0 = floor(p / cubesize), ind1 = fmod(ceil(p / cubesize), size) (periodic; a
 * coordinate exactly on a node has ind1 == ind0), the weight of node ind0 is |p - (ind0 + 1) cubesize| / cubesize and that of
 * ind1 |p - ind0 cubesize| / cubesize; a corner's weight is (wx wy) wz and its term w * value, all fp32.  grid[channels,r0,r1,r2]
 * receives per node the fp64 sum of the terms that land on it (cells in a fixed order, points in ascending index, corners
 * ascending), rounded to fp32 once; weighted != 0 divides it (fp32) by the number of (point, corner) pairs on the node,
 * zero-weight pairs included, 0 replaced by 1.  counts[r0,r1,r2] i32 (NULL = not wanted) receives that number.  Waits on
 * `stream` once.  GSR_ERR_ARG for a coordinate that is not finite or outside [0, 1) (nothing is written then). */
int gsr_psr_rasterize(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, const float* values,
                      int channels, int r0, int r1, int r2, int weighted, float* grid, int* counts, void* stream);

/* The spectral Poisson solve of DPSR.forward (:305-316) in one pass: spectrum = rfftn of the rasterized normals,
 * [3, r0, r1, r2/2+1] complex64 (interleaved re, im); phi[r0, r1, r2/2+1] complex64.  Per element, with the integer
 * frequencies k of np.fft.fftfreq / rfftfreq: G = (float)exp(-0.5 (sig 2 |k| / r0)^2) in fp64; then in fp32 N_d = N_d G,
 * w_d = (k_d 2) pi, DivN = sum_d (Im N_d w_d, -Re N_d w_d), Lap = -sum_d w_d^2, phi = DivN / (Lap + 1e-6); phi[0,0,0] = 0. */
int gsr_psr_spectral(const float* spectrum, int r0, int r1, int r2, double sig, float* phi, void* stream);

/* grid_interp (:69-112) of grid[r0,r1,r2] at points[num_points,3] (the index and weight arithmetic of gsr_psr_rasterize):
 * samples[i] = the 8 terms grid[corner] * w (fp32) added in fp64 in the reference's corner order, rounded once.  mean[1]
 * (f64, device, NULL = not wanted) = the fp64 sum of the samples in a fixed order (per 256 points a fixed tree, then the
 * partial sums in a fixed tree) / num_points.  Waits on `stream` once.  GSR_ERR_ARG for a bad coordinate as above. */
int gsr_psr_interp(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grid, int r0, int r1, int r2, const float* points,
                   int num_points, float* samples, double* mean, void* stream);

/* The tail of DPSR.forward (:323-332) and the tanh of ShapeAsPoints.generate_mesh in one stream over `count` values, fp32:
 * v = in - (float)mean[0] when mean (f64[1], device) is given; then with scale != 0 v = -v / |v[0]| * 0.5, v[0] the first
 * value after the shift; then with apply_tanh != 0 v = tanh(v).  grid_out may be grid_in.  params: f32[2] device scratch. */
int gsr_psr_normalize(const float* grid_in, float* grid_out, long long count, const double* mean, int scale, int apply_tanh,
                      float* params, void* stream);

/* Dense indexed marching cubes over the (r0-1)(r1-1)(r2-1) cubes of grid[r0,r1,r2] (not periodic) with gsr_mc_tables.h: a
 * corner is inside iff value < level, triangle normals point towards increasing value.  Every edge between two nodes that
 * crosses the level carries one vertex, owned by the edge's lower node; a vertex lies at index + (level - a) / (b - a) (fp32,
 * a the owner's value) along its axis, in index units.  Vertices are ordered by (owner node linear index, axis), triangles by
 * (linear index of the cube's lower node, table order).  gsr_psr_mc_classify fills node_info[r0 r1 r2] (u32) and the two
 * exclusive scans vertex_offset / triangle_offset [r0 r1 r2 + 1] (i32), stores the counts in *num_vertices / *num_triangles
 * (HOST) and waits on `stream` once; gsr_psr_mc_emit writes vertices[num_vertices,3] f32 and faces[num_triangles,3] i32
 * (either may be NULL). */
int gsr_psr_mc_classify(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grid, int r0, int r1, int r2, float level,
                        uint32_t* node_info, int* vertex_offset, int* triangle_offset, int* num_vertices, int* num_triangles,
                        void* stream);
int gsr_psr_mc_emit(const float* grid, int r0, int r1, int r2, float level, const uint32_t* node_info, const int* vertex_offset,
                    const int* triangle_offset, float* vertices, int* faces, void* stream);

/* Vertex normals of the mesh of gsr_psr_mc_emit, from the node_info / vertex_offset of gsr_psr_mc_classify on the same grid and
 * level: normals[num_vertices,3] f32 in vertex order.  Per vertex the grid's gradient at the two end nodes of its edge
 * (central difference (g[i+1] - g[i-1]) * 0.5 per axis in index units, one-sided g[1] - g[0] / g[r-1] - g[r-2] on the faces
 * of the grid), n = ga + t (gb - ga) with the vertex's own t = (level - a) / (b - a), then n / max(|n|, 1e-6); all fp32. */
int gsr_psr_mc_normals(const float* grid, int r0, int r1, int r2, float level, const uint32_t* node_info, const int* vertex_offset,
                       float* normals, void* stream);

/* ---- The backward of the Shape-as-Points stages.  Additive to ABI 6.  The numeric contract is the
 * forward's: the fp32 index / weight chain, fp32 terms added in fp64 in a fixed order and rounded once, no float atomics,
 * bit-identical from run to run, GSR_ERR_ARG for a coordinate that is not finite or outside [0, 1).  Derivative rule: a
 * weight factor |p - pos| / cubesize differentiates to sign(p - pos) / cubesize (fp32) with sign(0) = 0; floor, ceil and
 * the pair counts contribute nothing.  dw_kd below is the weight of corner k with the factor of axis d so replaced. ---- */

/* Backward of gsr_psr_rasterize, one lane per point: grad_grid[channels,r0,r1,r2], counts[r0,r1,r2] = the forward's counts
 * (read only when weighted; g' = g / (float)max(count, 1), else g' = g).  grad_values[n,c] = sum_k (w_k g'[c,node_k]),
 * grad_points[n,d] = sum_c sum_k ((dw_kd g'[c,node_k]) values[n,c]); corners k = (k0,k1,k2), k0 slowest.  Either output may
 * be NULL.  Waits on `stream` once. */
int gsr_psr_rasterize_bwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grad_grid, const float* points,
                          int num_points, const float* values, int channels, int r0, int r1, int r2, int weighted,
                          const int* counts, float* grad_values, float* grad_points, void* stream);

/* Backward of gsr_psr_interp towards the points: grad_points[n,d] = sum_k ((grid[node_k] dw_kd) grad_samples[n]).  The
 * gradient towards the grid is the adjoint scatter gsr_psr_rasterize(points, grad_samples, channels = 1, weighted = 0).
 * Waits on `stream` once. */
int gsr_psr_interp_bwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grid, int r0, int r1, int r2,
                       const float* points, int num_points, const float* grad_samples, float* grad_points, void* stream);

/* Backward of gsr_psr_spectral in PyTorch's convention for complex gradients: grad_phi[r0,r1,r2/2+1] complex64 ->
 * grad_spectrum[3,r0,r1,r2/2+1] complex64, grad_N_d = conj(c_d) grad_phi with c_d = -i w_d G / (Lap + 1e-6), zero at
 * element 0.  fp32 chain: a = grad_phi / (Lap + 1e-6), (-Im a w_d, Re a w_d), times G (fp64, cast, as in the forward). */
int gsr_psr_spectral_bwd(const float* grad_phi, int r0, int r1, int r2, double sig, float* grad_spectrum, void* stream);

/* Backward of gsr_psr_normalize: grid_out = the forward's output (read only with apply_tanh), params = the forward's params
 * (|v[0]| is a constant: the reference detaches it).  In fp32 grad_in = grad_out (1 - out^2) with apply_tanh, then
 * -grad_in / |v[0]| * 0.5 with scale.  grad_mean[1] (f64, device, NULL = not wanted) = -(fixed-order fp64 sum of grad_in). */
int gsr_psr_normalize_bwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grad_out, const float* grid_out,
                          long long count, const float* params, int scale, int apply_tanh, float* grad_in, double* grad_mean,
                          void* stream);

/* ---- visual hull (csrc/gsr_hull.hip): the `VisualHull` initializer's carve, gaustudio/pipelines/initializers/mask.py:38-71 ----
 * A camera of the carve: m = full_proj_transform as the reference stores it (row-vector convention, row-major [4][4]:
 * clip_c = ((x m[c] + y m[4+c]) + z m[8+c]) + m[12+c]); the view's packed mask starts at word_offset of mask_words and has
 * row_stride words per row (bit x & 31 of word x >> 5 is pixel x).  has_mask = 0: every voxel inside the view is kept. */
typedef struct gsr_hull_camera {
	float m[16];
	int32_t width, height;
	uint32_t word_offset;
	int32_t row_stride;
	int32_t has_mask;
	int32_t reserved[3];
} gsr_hull_camera;

/* Packs mask[height,width] (dtype 0: one byte per pixel, uint8 or bool; 1: float32; a pixel is set iff its value is nonzero,
 * NaN included) into bits at mask_words + word_offset: row y starts at word y * row_stride (row_stride >= ceil(width / 32);
 * the bits of a row's last word beyond `width` are 0, words of a wider stride are not written).  GSR_ERR_ARG unless
 * word_offset + height * row_stride <= num_words. */
int gsr_hull_pack_masks(const void* mask, int dtype, int width, int height, uint32_t* mask_words, uint64_t word_offset, int row_stride,
                        uint64_t num_words, void* stream);

/* Carves the grid [r0,r1,r2] (r0 r1 r2 < 2^31): voxel (i,j,k), flat index (i r1 + j) r2 + k, sits at (axis_x[j], axis_y[i],
 * axis_z[k]) (np.meshgrid's 'xy' indexing; axis_x has r1, axis_y r0, axis_z r2 entries, device memory).  Per camera, in list
 * order, Camera.insideView (gaustudio/datasets/__init__.py:268-305): clip = [x,y,z,1] @ m in the order above, ndc = clip.xy /
 * clip.w, kept iff clip.z > 0, -1 <= ndc.x, ndc.y <= 1 and the mask bit at (min(max(int((ndc.x + 1) * 0.5f * width), 0),
 * width - 1), likewise y with (1 + ndc.y) and height) is set.  filled[t] (u8) = 1 iff every camera keeps the voxel; *count
 * (device u32, zeroed by the call) = number of filled voxels; carved_by[t] (i32, may be NULL) = the first camera that carved
 * the voxel, -1 for a filled one.  cameras_host[num_cameras] (HOST) is validated (GSR_ERR_ARG for a mask region outside
 * [0, num_words)) and copied to cameras_device on `stream`: keep it alive until the stream has passed the call (the caller reads *count anyway). */
int gsr_hull_carve(const float* axis_x, const float* axis_y, const float* axis_z, int r0, int r1, int r2,
                   const gsr_hull_camera* cameras_host, gsr_hull_camera* cameras_device, int num_cameras, const uint32_t* mask_words,
                   uint64_t num_words, uint8_t* filled, uint32_t* count, int* carved_by, void* stream);

/* ---- mesh voxelization (csrc/gsr_voxel.hip): the `VoxelInitializer`'s hot path, gaustudio/pipelines/initializers/mesh.py:252-442 ----
 * A triangle mesh (vertices[num_vertices,3] f64, faces[num_faces,3] i32, device memory) against the grid [n0,n1,n2] of cubic
 * voxels of edge voxel_size whose lower corner is min_bound[3] (HOST): 2 <= n_d <= GSR_VOXEL_MAX_RES, voxel_size > 0.  All
 * arithmetic is float64, operation for operation that of tests/mesh_voxel_model.py: Akenine-Moller's triangle / box test with
 * its exact comparisons (touching overlaps) around the box centre (min_bound + voxel_size / 2) + i voxel_size.  Arrays are
 * caller-owned device memory, scratch comes from the gsr_alloc_fn callback (once per call), `stream` is the HIP stream of every
 * launch, a count that sizes the next stage's arrays is written to HOST memory after one wait on `stream`.  The stages:
 *
 * gsr_voxel_plan:  validates the mesh -- GSR_ERR_ARG for a face index outside [0, num_vertices), a vertex coordinate that is
 *   not finite, a bad grid, or more than GSR_VOXEL_MAX_ITEMS work items, with nothing written to the caller's arrays -- and
 *   writes per triangle tri_box[num_faces,6] = (lo0, lo1, lo2, hi0, hi1, hi2), its inclusive index-space box widened by one
 *   voxel and clamped to the grid, and col_start[num_faces + 1], the exclusive scan of its number of (i0, i1) columns.
 *   *num_items = the number of (triangle, column) work items.
 * gsr_voxel_count: item_start[num_items + 1] = exclusive scan of the overlaps of each work item; *num_pairs = their number
 *   (GSR_ERR_ARG beyond GSR_VOXEL_MAX_ITEMS).  A work item tests only the i2 range its triangle's plane can reach in the
 *   column, one voxel wider either side (the whole box range when the normal's component along i2 is too small to bound the
 *   error): a filter, the overlap test alone decides.
 * gsr_voxel_emit:  pair_voxel[num_pairs] (linear index (i0 n1 + i1) n2 + i2) and pair_tri[num_pairs] in work-item order
 *   (triangles ascending).  No wait.
 * gsr_voxel_sort:  stable radix sort of the pairs by voxel (only the digits n0 n1 n2 needs), head flags, scan:
 *   voxel_index[num_voxels] ascending, pair_start[num_voxels + 1], pair_tri[num_pairs] (triangles ascending within a voxel),
 *   and, when not NULL, grid_index[num_voxels,3] and occupancy[ceil(n0 n1 n2 / 32)] (bit t & 31 of word t >> 5; zeroed by the
 *   call).  Size voxel_index / pair_start / grid_index for num_pairs voxels; *num_voxels says how many there are.
 * gsr_voxel_closest: per occupied voxel, Ericson's closest point on a triangle from the voxel centre ((i + 0.5) voxel_size) +
 *   min_bound over the triangles listed in the 27 voxels around it: closest_tri[num_voxels] (smallest d2, exact ties to the
 *   lower triangle, a d2 that is not finite never wins; -1 = none), closest_uvw[num_voxels,3] f64 = (1 - v - w, v, w) (0 for
 *   -1) and, when color is not NULL, color[num_voxels,3] f32 = c0 u + c1 v + c2 w in f64 of vertex_colors[num_vertices,3] f32,
 *   rounded once (0.5 for -1).  A listed triangle or face index out of range is skipped.  No wait.
 * Bit-identical from run to run (no float atomics). */
#define GSR_VOXEL_MAX_RES 1024
#define GSR_VOXEL_MAX_ITEMS (1 << 30)
int gsr_voxel_plan(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const double* vertices, int num_vertices, const int* faces,
                   int num_faces, double voxel_size, const double* min_bound, int n0, int n1, int n2, int* tri_box, int* col_start,
                   int* num_items, void* stream);
int gsr_voxel_count(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const double* vertices, const int* faces, int num_faces,
                    double voxel_size, const double* min_bound, int n0, int n1, int n2, const int* tri_box, const int* col_start,
                    int num_items, int* item_start, int* num_pairs, void* stream);
int gsr_voxel_emit(const double* vertices, const int* faces, int num_faces, double voxel_size, const double* min_bound, int n0, int n1,
                   int n2, const int* tri_box, const int* col_start, int num_items, const int* item_start, uint32_t* pair_voxel,
                   int* pair_tri, void* stream);
int gsr_voxel_sort(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const uint32_t* pair_voxel, const int* pair_tri_in, int num_pairs,
                   int n0, int n1, int n2, uint32_t* voxel_index, int* pair_start, int* pair_tri, int* grid_index, uint32_t* occupancy,
                   int* num_voxels, void* stream);
int gsr_voxel_closest(const double* vertices, int num_vertices, const int* faces, int num_faces, const float* vertex_colors,
                      double voxel_size, const double* min_bound, int n0, int n1, int n2, const uint32_t* voxel_index,
                      const int* pair_start, const int* pair_tri, int num_voxels, int* closest_tri, double* closest_uvw, float* color,
                      void* stream);

/* ---- vertex-colour baking and per-triangle Gaussian seeds: the per-view body of gaustudio/scripts/texture_mesh.py:108-141
 * and MeshInitializer.build_model (gaustudio/pipelines/initializers/mesh.py:20-250) for a mesh that stays in HBM.  Additive
 * to ABI 6, in the style of gsr_mesh_*: inputs and outputs are caller-owned device memory, `stream` is the HIP stream of
 * every launch, intrinsics (3x3 row-major K; fx, fy, cx, cy are read) and extrinsics (4x4 row-major world-to-camera, OpenCV
 * axes) are HOST pointers.  float32 throughout, correctly rounded divide / sqrt; no FMA in the two bake entries, the explicit
 * ones named below in gsr_mesh_seeds; deterministic (no atomics on any result).  Contract: INTEGRATION.md s21; design: gsr_mesh_bake.hip, DESIGN.md s18. ---- */

/* One view's facing filter.  For every face with visible[f] != 0 (u8, gsr_mesh_visible_faces): n = (v1 - v0) x (v2 - v0),
 * cos = (n / |n|) . d with d the normalised third row of the world-to-camera rotation; cos < -0.05f selects the face and
 * writes stamp[v] = seq (seq >= 0) for its three vertices, by plain stores.  stamp[num_verts] i32 is the caller's, set to -1
 * once per bake, never cleared between views.  cos_out[num_faces] f32 (may be NULL) receives cos, NaN for a face that is not
 * visible.  A degenerate face (|n| = 0: cos = NaN) and a face with an index outside [0, num_verts) select nothing.  No wait.
 * GSR_ERR_ARG for a non-finite matrix or a viewing axis without length. */
int gsr_mesh_bake_select(const float* verts, int num_verts, const int* faces, int num_faces, const unsigned char* visible,
                         const float extrinsics[16], int seq, int* stamp, float* cos_out, void* stream);

/* One view's colour lookup, for every vertex with stamp[v] == seq.  image[height,width,3] f32 (device).  exact == 0, the
 * reference: x = (fx (-x_c)) / z_c + cx, y likewise (PyTorch3D's screen camera after the script's RDF->LUF flip: 2 cx - u),
 * g_x = 2 (x / (width - 1)) - 1, g_y = 2 (y / (height - 1)) - 1, valid when both lie in [-1, 1]; then grid_sample(bilinear,
 * align_corners=False, padding reflection) of the image flipped in both axes: i_x = ((g_x + 1) width - 1) / 2 clipped to
 * [0, width - 1], four taps summed in nw, ne, sw, se order, a tap at column `width` or row `height` skipped.  exact != 0:
 * u = (fx x_c) / z_c + cx, v likewise, valid when 0 <= u <= width and 0 <= v <= height, the unflipped image sampled at column
 * u - 0.5, row v - 0.5 by the same rule.  A valid vertex writes colors[v] (3 f32, clamped to [0, 1]) and baked_by[v] = seq;
 * every other entry of colors[num_verts,3] / baked_by[num_verts] stays as it is.  z_c is not tested (a vertex behind the
 * camera can be valid, as in the reference).  No wait.  GSR_ERR_ARG for a bad size (> 16384) or singular intrinsics. */
int gsr_mesh_bake_sample(const float* verts, int num_verts, const int* stamp, int seq, const float intrinsics[9],
                         const float extrinsics[16], const float* image, int height, int width, int exact, float* colors,
                         int* baked_by, void* stream);

/* MeshInitializer.build_model: n_per_triangle (1, 3, 4 or 6) flat Gaussians per face, Gaussian g = f * n + k.  With the
 * barycentric table b_k of mesh.py:98-137: xyz = (b0 v0 + b1 v1) + b2 v2; f_dc = (rgb - 0.5) / C0 with rgb the same sum of
 * vertex_colors, or 1 when vertex_colors is NULL; scale = (l, l, log(1e-7)) with l = log(2 s + 1e-7), s = max(min edge
 * length * radius_n, 0), each logarithm float(log(double(x))); rot = rotmat2quaternion(normal2rotation(N)) (w, x, y, z; not
 * normalised) of N = the same sum of normals[num_verts,3], normalised twice with x / max(|x|, 1e-12), torch.cross taken along
 * the last axis.  In this entry every norm is |x| = sqrt(fma(x.z, x.z, fma(x.y, x.y, x.x * x.x))) (the edge lengths and the three
 * normalisations) and the cross product is a x b = (fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)),
 * fma(a.x, b.y, -(a.y * b.x))), the forms torch's CPU kernels evaluate; every other operation is a single float32 operation
 * in the order written in INTEGRATION.md s21.  Outputs xyz / f_dc / scale [num_faces * n, 3] and rot [num_faces * n, 4] f32.  Waits on `stream` once;
 * GSR_ERR_ARG for another n_per_triangle, num_faces * n >= 2^31 or a face index outside [0, num_verts). */
int gsr_mesh_seeds(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, const float* normals,
                   const float* vertex_colors, int num_verts, const int* faces, int num_faces, int n_per_triangle, float* xyz,
                   float* f_dc, float* scale, float* rot, void* stream);

/* ---- Gaussian seeds from a point cloud: what every point-cloud initializer of the reference ends in
 * (VanillaPointCloud.create_from_attribute, gaustudio/models/vanilla_sg.py:69-97, with simple-knn's distCUDA2 /
 * calculate_dist2_python for scale=None), and DepthInitializer's float16 packing.  Additive to ABI 6, in the style of gsr_knn /
 * gsr_mesh_seeds.  Contract: INTEGRATION.md s22; design: gsr_knn.hip, gsr_mesh_bake.hip, DESIGN.md s19. ---- */

/* out_dist2[i] (f32) = (float)(((d1 + d2) + d3) / 3.0) with d1 <= d2 <= d3 the three smallest squared distances from point i to
 * the OTHER points (another index; a duplicate coordinate counts, at 0), each dx*dx + dy*dy + dz*dz in f64 from the f32
 * coordinates, summed in that order.  Only values enter: fully determined, bit-identical from run to run.  4 <= num_points
 * (GSR_ERR_ARG otherwise); GSR_ERR_NONFINITE for a NaN or infinite coordinate.  stats (HOST, may be NULL) receives {occupied grid
 * cells, lanes that scanned the second shell, points answered by the wave-per-query fallback}.  Waits on `stream` a few times
 * (the grid's cell counts, the fallback count). */
int gsr_mean_dist3(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, float* out_dist2,
                   int stats[3], void* stream);
/* The same with the measuring knobs: cell_target = points per occupied grid cell the build aims at (0 = the library's default,
 * at most 64; the result does not depend on it); stage_ms (HOST, may be NULL) receives the GPU milliseconds of {grid build,
 * lane-per-point query, fallback including the host's read of its count} from HIP events on `stream`. */
int gsr_mean_dist3_ex(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, float* out_dist2,
                      int cell_target, int stats[3], float stage_ms[3], void* stream);

/* create_from_attribute, one lane per point, f32 throughout.  xyz_out = xyz; f_dc = (rgb - 0.5f) / C0, rgb = 1 when NULL;
 * scale = scale_in, or when that is NULL all three axes float(log(double(sqrtf(dist2[i] + 1e-7f)))) (exactly one of dist2 /
 * scale_in is given); rot = rot_in, or rotmat2quaternion(normal2rotation(normals)) in gsr_mesh_seeds' arithmetic with one
 * x / max(|x|, 1e-12), or (1, 0, 0, 0) when both are NULL (both given: GSR_ERR_ARG); opacity_out = opacity_in [n], or the scalar
 * `opacity` when NULL.  Inputs [n,3] ([n,4] rot_in); outputs xyz_out / f_dc / scale [n,3], rot [n,4], opacity_out [n].  No wait. */
int gsr_point_seeds(const float* xyz, const float* rgb, const float* dist2, const float* scale_in, const float* rot_in,
                    const float* normals, const float* opacity_in, float opacity, int num_points, float* xyz_out, float* f_dc,
                    float* scale, float* rot, float* opacity_out, void* stream);

/* One frame of DepthInitializer (gaustudio/pipelines/initializers/depth.py:50-89) without its files: per pixel
 * xyz = float(half(points)); rgb = float(uint8(half(half(image) * 255))) / 255.0f (colours in [0, 1]; negative or NaN ones are
 * outside the contract); scale (three equal axes) = float(half(float(log(double(s))))), s = float(half(depth / focal)), focal =
 * (fx + fy) / 2 in f32: a depth of 0 gives -inf.  points / image [n,3], depth [n]; outputs [n,3].  No wait. */
int gsr_depth_seed_pack(const float* points, const float* image, const float* depth, int num_pixels, float focal, float* xyz,
                        float* rgb, float* scale, void* stream);

/* ---- Scaffold-GS inference in front of the operator (csrc/gsr_scaffold.hip): gaustudio/renderers/scaffold_renderer.py
 * get_gaussians_properties with its prefilter_voxel, fused into two passes over the anchors.  Additive to ABI 6.  Contract:
 * INTEGRATION.md s23 (and its definition, tests/scaffold_model.py); design: DESIGN.md s20.  Device memory, f32, contiguous:
 * anchor [N,3], anchor_feat [N,32], offset [N,k,3], scaling [N,6] and rot [N,4] (both activated), viewmatrix / projmatrix [16]
 * and campos [3] with the operator's conventions.  weights (HOST array of 16 device pointers): W1, b1, W2, b2 (nn.Linear
 * layout, W [out,in]) of the opacity MLP (36 -> 32 -> k), the covariance MLP (36 -> 32 -> 7k), the colour MLP (36 -> 32 -> 3k)
 * and the feature bank (4 -> 32 -> 3; four NULLs = no bank).  1 <= k <= 16, 0 <= N <= 2^24, N k < 2^31 (GSR_ERR_ARG).
 * Every dot product is bias first, then fma over the ascending input index; bit-identical from run to run. ---- */

/* Pass 1.  visible[a] (u8) = visible_in[a] != 0 when visible_in is given; otherwise radii[a] (i32) = the radius gsr_forward
 * reports for a Gaussian at anchor[a] with scales scaling[a,0:3] * scale_modifier and rotation rot[a] (0 for a culled one)
 * and visible[a] = radii[a] > 0 (radii is not written when visible_in is given).  kept[a] (u16): bit j set iff the anchor is
 * visible and logit j of the opacity MLP is > 0 (a NaN is not).  start[N + 1] (i32): exclusive scan of the bit counts;
 * *total (HOST) = start[N], read after one wait on `stream`.  Scratch from the allocator callback, once. */
int gsr_scaffold_count(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* anchor, const float* anchor_feat,
                       const float* scaling, const float* rot, const float* const weights[16], int num_anchors, int n_offsets,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tanfovx, float tanfovy,
                       int image_width, int image_height, float scale_modifier, const unsigned char* visible_in,
                       unsigned char* visible, int* radii, unsigned short* kept, int* start, int* total, void* stream);

/* Pass 2.  For every set bit (a, j) of kept, at row start[a] + (number of set bits of kept[a] below j) -- anchor-major,
 * offset-minor: xyz [M,3] = anchor + offset[a,j] * scaling[a,0:3]; opacity [M] = tanh(logit); colors [M,3] = sigmoid; scales
 * [M,3] = scaling[a,3:6] * sigmoid(o[0:3]); rotations [M,4] = o[3:7] / max(|o[3:7]|, 1e-12); anchor_index / offset_index [M]
 * i32.  tanh and sigmoid from the library's polynomial exp.  num_gaussians = *total of pass 1; an
 * anchor whose rows would not fit [0, num_gaussians) writes nothing.  No wait. */
int gsr_scaffold_emit(const float* anchor, const float* anchor_feat, const float* offset, const float* scaling,
                      const float* const weights[16], int num_anchors, int n_offsets, const float* campos, const unsigned short* kept,
                      const int* start, int num_gaussians, float* xyz, float* colors, float* opacity, float* scales, float* rotations,
                      int* anchor_index, int* offset_index, void* stream);

/* The gradient of the two passes above (its definition: tests/scaffold_grad_model.py; design: DESIGN.md
 * s20a).  kept / start / num_gaussians: what pass 1 returned for the same inputs; the forward values are recomputed from them
 * by the forward's own code.  g_xyz [M,3], g_colors [M,3], g_opacity [M], g_scales [M,3], g_rotations [M,4]: the cotangents of
 * pass 2's outputs in its row order, contiguous; NULL = zeros.  Outputs, all written (zero rows for invisible anchors, for
 * anchors without a kept offset and for dropped offsets): d_anchor [N,3], d_anchor_feat [N,32], d_offset [N,k,3], d_scaling
 * [N,6]; d_weights (HOST array of 16 device pointers, laid out as `weights`, the bank's four NULL iff the bank's are): the
 * gradients of W1, b1, W2, b2 of each MLP.  The visible mask, the kept mask, rot, campos and the camera are constants.  The
 * sums over anchors follow a fixed tree (256-anchor blocks dealt to 256 chains, block b to chain b mod 256; ascending within
 * a chain; the chains added in ascending order in f64): no atomics, bit-identical from run to run and on any stream.  With
 * num_gaussians == 0 no kernel is launched and every output is zero.  Scratch from the allocator callback, once: at most
 * 65536 anchors are staged at a time.  No wait. */
int gsr_scaffold_backward(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* anchor, const float* anchor_feat,
                          const float* offset, const float* scaling, const float* const weights[16], int num_anchors, int n_offsets,
                          const float* campos, const unsigned short* kept, const int* start, int num_gaussians, const float* g_xyz,
                          const float* g_colors, const float* g_opacity, const float* g_scales, const float* g_rotations,
                          float* d_anchor, float* d_anchor_feat, float* d_offset, float* d_scaling, float* const d_weights[16],
                          void* stream);

/* ---- The photometric loss of 3DGS training (csrc/gsr_loss.hip): loss = (1 - lambda) L1 + lambda (1 - SSIM), SSIM with the
 * 11 x 11 Gaussian window (sigma 1.5) under zero padding.  Additive to ABI 6.  Contract, float order included: INTEGRATION.md
 * s24 (its definition to the bit: tests/loss_model.py); design: DESIGN.md s21.  image / target: device, f32, contiguous,
 * [planes, height, width].  planes, height, width >= 1 and planes * height * width < 2^31, 0 <= lambda_dssim <= 1
 * (GSR_ERR_ARG otherwise).  No atomics: bit-identical from run to run and on any stream.  No wait. ---- */

/* out3 (device) = {loss, l1, ssim} as f32, formed in f64 from per-workgroup f64 partials (scratch from the allocator callback,
 * once).  ssim_map [planes,H,W] (may be NULL) receives the per-pixel SSIM; maps [3,planes,H,W] (may be NULL: forward only)
 * receives what gsr_photometric_bwd convolves. */
int gsr_photometric_fwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* image, const float* target,
                        long long planes, int height, int width, float lambda_dssim, float* ssim_map, float* maps, float* out3,
                        void* stream);
/* grad_image [planes,H,W] = *grad_loss * d loss / d image, from the maps of a forward on the same image and target.
 * grad_loss: one f32 in DEVICE memory, the upstream gradient of the scalar loss. */
int gsr_photometric_bwd(const float* image, const float* target, const float* maps, long long planes, int height, int width,
                        float lambda_dssim, const float* grad_loss, float* grad_image, void* stream);

/* ---- The geometric regularisers of 2D Gaussian surfel training (csrc/gsr_geoloss.hip): loss = lambda_normal mean(1 - <N, n a1>)
 * + lambda_dist mean(a6) on the surfel operator's allmap [7,height,width] (device, f32, contiguous), n the normal of the
 * blended depth (1 - depth_ratio) nan_to_num(a0 / a1) + depth_ratio nan_to_num(a5) by central differences of the camera-space
 * points, 0 on the one-pixel border.  Additive to ABI 6.  Contract, float order included: INTEGRATION.md s26 (its definition
 * to the bit: tests/geoloss_model.py); design: DESIGN.md s23.  height, width >= 1 and 7 * height * width < 2^31,
 * 0 <= depth_ratio <= 1, lambdas finite and >= 0, fx, fy, cx, cy finite, fx and fy non-zero (GSR_ERR_ARG otherwise).  No atomics:
 * bit-identical from run to run and on any stream.  No wait. ---- */

/* out3 (device) = {loss, normal_loss, dist_loss} as f32, formed in f64 from per-workgroup f64 partials (scratch from the allocator
 * callback, once).  maps [10,H,W] (may be NULL) receives {expected depth, median depth, blended depth, n a1 (3 planes), the
 * rendered normal (3 planes), 1 - <N, n a1>}; viewmatrix (device, 16 floats as the operator takes it, may be NULL) turns the two
 * normals of `maps` to world space, v -> sum_i v_i viewmatrix[4 j + i].  The loss does not depend on it. */
int gsr_surfel_geoloss_fwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* allmap, int height, int width, float fx,
                           float fy, float cx, float cy, float depth_ratio, float lambda_normal, float lambda_dist,
                           const float* viewmatrix, float* maps, float* out3, void* stream);
/* grad_allmap [7,H,W] = *grad_loss * d loss / d allmap, every plane written; nothing is taken from a forward.  a1 is a constant
 * in the factor n a1; a pixel whose a0 / a1 is not finite gets 0 in planes 0 and 1, one whose a5 is not finite 0 in plane 5.
 * grad_loss: one f32 in DEVICE memory, the upstream gradient of the scalar loss. */
int gsr_surfel_geoloss_bwd(const float* allmap, int height, int width, float fx, float fy, float cx, float cy, float depth_ratio,
                           float lambda_normal, float lambda_dist, const float* grad_loss, float* grad_allmap, void* stream);

/* Per-stage GPU time, averaged over every gsr_forward / gsr_backward call made in this process (any thread) since
 * gsr_set_profiling(1): milliseconds for {preprocess, scan (tile histogram + scans + row offsets), scatter, sort, composite} (forward)
 * or {composite_bwd, preprocess_bwd} (backward), measured with HIP events recorded on the launch stream.
 * Recording costs one event per stage boundary (nine per forward + backward: ~3 % of a 1-ms step) and no synchronisation; the
 * getters synchronise on the last recorded event and return the number of calls averaged (0 = nothing recorded).
 * gsr_set_profiling(2) records the two boundaries of composite_fwd only (the other stages then read 0); 0 switches it off. */
void gsr_set_profiling(int enable);
int gsr_last_forward_ms(float ms[5]);
int gsr_last_backward_ms(float ms[2]);

/* ---- The optimiser step and adaptive density control of 3DGS training (csrc/gsr_optim.hip).  Additive to ABI 6.  Contract,
 * float order included: INTEGRATION.md s25 (its definition to the bit: tests/optim_model.py); design: DESIGN.md s22.
 * Every tensor: device, 4-byte elements, contiguous, [num_rows, width].  0 <= num_rows and num_rows * 45 < 2^31, widths
 * within [0, 45] (GSR_ERR_ARG otherwise).  No atomics: bit-identical from run to run and on any stream. ---- */

/* One parameter group of gsr_adam_step (HOST).  grad NULL or width 0: the group is skipped. */
typedef struct gsr_adam_group {
	float* param;
	const float* grad;
	float* exp_avg;
	float* exp_avg_sq;
	double lr;
	int width;
	int reserved;
} gsr_adam_group;

/* One launch for all groups: torch.optim.Adam without weight decay or amsgrad at step `step` >= 1 (the caller counts).  The
 * per-group constants 1 - beta1, 1 - beta2, sqrt(1 - beta2^step) and lr / (1 - beta1^step) are formed here in f64, rounded to
 * f32 once and passed to the kernel by value; nothing reads the device.  visible (device, int32 [num_rows], may be NULL): rows
 * with visible <= 0 keep parameter and both moments.  1 <= num_groups <= 6.  No wait. */
int gsr_adam_step(const gsr_adam_group* groups, int num_groups, int num_rows, double beta1, double beta2, double eps,
                  long long step, const int* visible, void* stream);

/* Rows with radii > 0: grad_accum += sqrt(gx gx + gy gy) of means2d_grad [num_rows,3], denom += 1, max_radii = max(max_radii,
 * radii).  No wait. */
int gsr_density_accumulate(int num_rows, const float* means2d_grad, const int* radii, float* grad_accum, int* denom,
                           int* max_radii, void* stream);

/* The classify and scan half of a compaction.  pos (device, int32 [3 num_rows + 1]) receives the exclusive scan of the three
 * per-row flags {the source survives, its clone is emitted, its children are emitted}, laid out flag-major, so that pos[i],
 * pos[num_rows + i] and pos[2 num_rows + i] + c * (pos[3 num_rows] - pos[2 num_rows]) are the output rows of source i, of its
 * clone and of its child c.  prune_mask (device, u8 [num_rows]) non-NULL: a plain prune -- a source survives where the mask is
 * 0 and nothing else is read.  Otherwise the densification of INTEGRATION.md s25 with thresholds formed here in f64;
 * max_screen_size < 0: no screen- and world-size tests.  totals_host[4] (HOST) = {survivors, clones, split sources with
 * children, rows after}.  Waits on `stream` once, for the totals; GSR_ERR_ARG, nothing else written, when rows after * 45
 * >= 2^31.  Scratch from the allocator callback, once. */
int gsr_densify_classify(gsr_alloc_fn workspace_alloc, void* workspace_ctx, int num_rows, const float* scaling,
                         const float* opacity, const float* grad_accum, const int* denom, const int* max_radii,
                         const unsigned char* prune_mask, float max_grad, double percent_dense, double extent,
                         double min_opacity, int max_screen_size, int n_split, int* pos, long long* totals_host, void* stream);

#define GSR_COMPACT_COPY 0     /* the value goes to every output row of its source; moments: carried by the survivor, else 0 */
#define GSR_COMPACT_XYZ 1      /* as COPY, a child gets xyz + R(q / |q|) (exp(scaling) * noise) */
#define GSR_COMPACT_SCALING 2  /* as COPY, a child gets scaling - log(0.8 n_split) */
#define GSR_COMPACT_STATS 3    /* three per-row statistics, carried by survivors only (their other rows are not written) */

/* One group of gsr_densify_emit (HOST): a parameter with its two moments (or three statistics), source and destination. */
typedef struct gsr_compact_group {
	const void* src[3];
	void* dst[3];
	int width;
	int kind;
} gsr_compact_group;

/* The emit half: one launch writes every destination row of every group from `pos`.  noise: f32 [num_rows, n_split, 3] by
 * SOURCE row, read for rows with children only (may be NULL when pos holds none).  scaling / rotation: the source tensors the
 * children's positions are formed from.  Sources are never written.  1 <= num_groups <= 8.  No wait. */
int gsr_densify_emit(int num_rows, int n_split, const gsr_compact_group* groups, int num_groups, const int* pos,
                     const float* noise, const float* scaling, const float* rotation, void* stream);

/* ---- Scaffold-GS anchor control: the statistics, anchor growing by voxel level and pruning as one compaction that carries
 * the Adam moments (csrc/gsr_anchor.hip).  Additive to ABI 6.  Contract to the bit: INTEGRATION.md s23b (its definition:
 * tests/anchor_model.py); design: DESIGN.md s20b.  Every tensor: device, 4-byte elements, contiguous.  0 <= num_anchors
 * <= 2^24, 1 <= k <= 16 (GSR_ERR_ARG otherwise).  No float atomics: bit-identical from run to run and on any stream. ---- */
#define GSR_ERR_CELL (-7)        /* gsr_anchor_level: a candidate's position is not finite or its cell does not fit 21 bits */
#define GSR_ANCHOR_FEAT 32       /* floats of an anchor_feat row */
#define GSR_ANCHOR_MAX_LEVELS 8  /* levels of one pass */

/* One launch.  Gaussian m < num_gaussians with radii[m] > 0: slot = anchor_index[m] k + offset_index[m] gets offset_grad_accum
 * += sqrt(gx gx + gy gy) of viewspace_grad [num_gaussians,3] and offset_denom += 1.  Anchor a with visible[a] (u8): anchor_denom
 * += 1.  The first Gaussian of an anchor's run (runs are contiguous, anchor-major): opacity_accum[a] += the f32 sum of the run's
 * opacities in order.  A Gaussian whose indices are out of range is skipped.  No wait. */
int gsr_anchor_accumulate(int num_anchors, int k, int num_gaussians, const int* anchor_index, const int* offset_index,
                          const float* opacity, const float* viewspace_grad, const int* radii, const unsigned char* visible,
                          float* offset_grad_accum, int* offset_denom, float* opacity_accum, int* anchor_denom, void* stream);

/* The new anchors of an earlier level of the same pass (HOST): their cells (device, int32 [count,3]) and the voxel size they
 * were formed with; their positions are f32(cell) * cur. */
typedef struct gsr_anchor_cells {
	const int* cells;
	int count;
	float cur;
} gsr_anchor_cells;

/* One level of growing.  A slot (a, j) is a candidate when offset_denom > mature_min, avg = accum / f32(denom) >= grad_min and
 * rand [num_anchors k] > rand_min.  Its position is anchor + offset * gs_exp(clamp(scale_raw[a, 0:3], -80, 80)), its cell
 * rintf(position / cur).  The new anchors of the level are the distinct candidate cells that hold neither one of the
 * num_anchors anchors nor one of prior[num_prior] (cells formed the same way, at this level's cur), in ascending (x, y, z)
 * order.  The allocator is called up to three times: scratch twice, then ONE block that the caller keeps until its emit: the
 * cells int32 [count,3] at *cells_out and, behind them, the per-cell maximum of the candidates' anchor_feat rows, f32
 * [count,32], at *feat_out (both NULL when count is 0).  info_host[2] (HOST) = {candidates, count}.  Waits on `stream` twice:
 * for the candidate count with the cell range (the sort's key width comes from it), and for the count.  GSR_ERR_CELL, nothing
 * allocated for the caller, for a candidate out of range. */
int gsr_anchor_level(gsr_alloc_fn workspace_alloc, void* workspace_ctx, int num_anchors, int k, const float* anchor,
                     const float* offset, const float* scale_raw, const float* anchor_feat, const float* offset_grad_accum,
                     const int* offset_denom, const float* rand, int mature_min, float grad_min, float rand_min, float cur,
                     const gsr_anchor_cells* prior, int num_prior, int** cells_out, float** feat_out, long long* info_host,
                     void* stream);

/* The prune decision and its scan: pos (device, int32 [num_anchors + 1]) = exclusive scan of "anchor a survives", i.e. not
 * (anchor_denom > settled_min and opacity_accum < min_opacity * f32(anchor_denom)).  *survivors_host (HOST) = pos[num_anchors].
 * Waits on `stream` once.  Scratch from the allocator callback, once. */
int gsr_anchor_prune(gsr_alloc_fn workspace_alloc, void* workspace_ctx, int num_anchors, const float* opacity_accum,
                     const int* anchor_denom, int settled_min, float min_opacity, int* pos, int* survivors_host, void* stream);

/* One tensor of gsr_anchor_emit (HOST): `width` 4-byte words per anchor.  kind: 0 a parameter or a moment (copied),
 * 1 offset_grad_accum / offset_denom (0 where offset_denom > mature_min, when mature_min >= 0), 2 opacity_accum / anchor_denom
 * (0 where anchor_denom > settled_min). */
typedef struct gsr_anchor_tensor {
	const void* src;
	void* dst;
	int width;
	int kind;
} gsr_anchor_tensor;

#define GSR_ANCHOR_COPY 0
#define GSR_ANCHOR_SLOT_STAT 1
#define GSR_ANCHOR_ANCHOR_STAT 2
#define GSR_ANCHOR_MAX_TENSORS 19   /* five parameters with two moments each and four statistics */

/* The one write of every output tensor.  Survivor a of pos goes to row pos[a] of every tensors[t].dst, its statistics reset as
 * their kind says.  The new anchors of
 * levels[num_levels] follow in level order from row pos[num_anchors]: tensors[0 .. 4] are anchor, anchor_feat, offset,
 * scale_raw, rot_raw and get f32(cell) * cur, the level's feature rows (feat[l]: device, f32 [count,32]), 0, f32(log(cur))
 * six times and (1, 0, 0, 0); every further tensor gets 0.  Sources are never written.  No wait. */
int gsr_anchor_emit(int num_anchors, int k, const gsr_anchor_tensor* tensors, int num_tensors, const int* pos,
                    const int* offset_denom, const int* anchor_denom, int mature_min, int settled_min,
                    const gsr_anchor_cells* levels, const float* const* feat, int num_levels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_H_INCLUDED */
