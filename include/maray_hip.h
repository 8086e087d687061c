/*
 * maray_hip.h — C ABI of libmaray_hip.so: the MI355X (gfx950) per-pixel
 * expression evaluator that drops in behind maray's render surface.
 *
 * Every entry point cites the reference interface (advancedresearch/maray
 * 0.3.8) it replaces or mirrors.  Conventions:
 *   - plain pointers and sizes only; opaque handles are owned by the library
 *     and released with the matching *_free;
 *   - output buffers are owned and sized by the caller; inputs are borrowed
 *     for the duration of the call only;
 *   - every function returns 0 on success or a negative MARAY_E_* code and
 *     never throws/aborts across the boundary; maray_last_error() returns a
 *     thread-local message;
 *   - calls are blocking; a maray_ctx is bound to one device and is not
 *     thread-safe (multi-GPU = one ctx per device);
 *   - there is NO CPU fallback: the render entry points fail with
 *     MARAY_E_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef MARAY_HIP_H
#define MARAY_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "maray_tape.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    MARAY_OK = 0,
    MARAY_E_ARG = -1,        /* bad argument */
    MARAY_E_IO = -2,         /* file error (open/save return anyhow::Error) */
    MARAY_E_DECODE = -3,     /* bincode decode error */
    MARAY_E_ALIASED = -4,    /* scene depends on Cache id-aliasing (reference result is order dependent) */
    MARAY_E_CYCLE = -5,      /* Let variable defined in terms of itself (reference overflows its stack) */
    MARAY_E_APP_RANGE = -6,  /* App id outside Runtime.functions (reference panics, src/lib.rs:665) */
    MARAY_E_LIMIT = -7,      /* tape limits exceeded (slots / constants / y values) */
    MARAY_E_NO_DEVICE = -8,  /* no usable gfx950 device, or HIP runtime error */
    MARAY_E_HIP = -9,        /* HIP runtime / hiprtc error */
    MARAY_E_INTERNAL = -10
};

const char *maray_last_error(void);
const char *maray_version(void);

/* ---- scene files ------------------------------------------------------------
 * `open` (src/lib.rs:1227-1235) / `save` (src/lib.rs:1216-1224): bincode 1.3.3
 * default options of `([u32;2], [Expr;3])`.  The reader auto-detects the
 * current tag numbering (src/lib.rs:101-149) and the legacy one used by
 * data/chess.maray (no Arc variant; tags one lower): it accepts the numbering
 * that consumes the buffer exactly. */
typedef struct maray_scene maray_scene;

int maray_scene_open(const char *path, maray_scene **out);
int maray_scene_from_bytes(const uint8_t *buf, size_t len, maray_scene **out);
void maray_scene_free(maray_scene *s);
int maray_scene_size(const maray_scene *s, uint32_t *w, uint32_t *h);
int maray_scene_set_size(maray_scene *s, uint32_t w, uint32_t h);
int maray_scene_is_legacy(const maray_scene *s, int *legacy);
/* Tree node count of channel c (definitions of Let variables counted once). */
int maray_scene_node_count(const maray_scene *s, int c, uint64_t *n);
/* `save`: encode in the current numbering.  *len_out = bytes needed; writes
 * only if cap is large enough. */
int maray_scene_encode(const maray_scene *s, uint8_t *out, size_t cap, size_t *len_out);
int maray_scene_save(const maray_scene *s, const char *path);
/* var_fixer::fix_color (src/var_fixer.rs:74-82).  maray_lower applies it
 * itself; exposed so the pre-pass can be tested on its own. */
int maray_scene_fix_color(maray_scene *s);
/* `Expr::scale`-style resampling (src/lib.rs:804-806) applied to the whole
 * scene including Let definitions: X -> X * (1/sx), Y -> Y * (1/sy), and the
 * header size multiplied by (sx, sy).  Exact when sx, sy are powers of two. */
int maray_scene_rescale(maray_scene *s, uint32_t sx, uint32_t sy);
/* `Expr::simplify` on each channel (src/lib.rs:601-604: constant_reduction at the root, src/constant_reduction.rs:9-185,
 * then the rewrite rules of src/simplify.rs:129-327).  Authoring-time, not on the render path; the reference applies it
 * before `save` (examples/chess.rs:43). */
int maray_scene_simplify(maray_scene *s);
/* The same with options.  MARAY_SIMPLIFY_MERGE_DIVISORS: one rewrite the reference does not have, `(a/p) * 1/q -> a / (p*q)`.
 * The reference's rules do not terminate on such a term -- src/simplify.rs:276-283 turns `(a/p) * 1/q` into `(a * 1/q) / p`,
 * whose numerator is the quotient a/q again, and the two divisors change places for ever (the reference overflows its
 * stack; maray_scene_simplify reports MARAY_E_LIMIT) -- and examples/chess.rs:43 builds such terms from every grid cell,
 * so the current revision cannot regenerate its own data/chess.maray (written by an older one: legacy tags, and naturals
 * that are products of such divisors).  With the flag the example's pipeline runs. */
enum { MARAY_SIMPLIFY_MERGE_DIVISORS = 1 };
int maray_scene_simplify_ex(maray_scene *s, uint32_t flags);
/* `Expr::compress` on each channel (src/lib.rs:610-614: `flatten`, src/compressor.rs:167-211, then the greedy
 * Let-introducing loop of `compress`, :214-236, driven by the printed length of every candidate term exactly as the
 * reference's `Display` prints it).  Changes no value.  n_vars3 (may be NULL): variables introduced per channel. */
int maray_scene_compress(maray_scene *s, uint32_t *n_vars3);
/* `format!("{}", color[c]).chars().count()` (impl Display for Expr, src/lib.rs:196-366): what compress weighs. */
int maray_scene_display_len(maray_scene *s, int c, uint64_t *len);

/* ---- scene parameters: a free variable gets its value at render time --------------------------------------------
 * A `Var` that no enclosing `Let` defines evaluates to NaN (src/cache.rs:32-40).  A scene may DECLARE such ids
 * (`var(name)`, src/lib.rs:845-850) as parameters: the lowering then keeps them as run-time operands (include/
 * maray_tape.h, SPEC PARAM), and a context takes new values between two launches -- the tape, the specialised kernels'
 * code objects, the contexts and everything gen_to_image keeps are reused from frame to frame.
 * Meaning: with parameter p = Var(id) set to v, the image is the one the reference renders for the scene in which every
 * occurrence of Var(id) that resolves to no definition at its use site (inside Let definitions too) is replaced by an
 * expression whose value is exactly v, bit for bit.  An occurrence a Let defines keeps its definition; a parameter that
 * was never set is NaN, i.e. the scene as it renders without the declaration.
 * The declared range [lo, hi] is what the lowering's static analysis works with (intervals, bounded Sin arguments,
 * guards); -inf, +inf means "anything, NaN included".  It is a promise that is checked: a value outside the range (or
 * NaN with any other range; -0.0 when the range starts at +0.0) is MARAY_E_ARG and the old value stays -- on the scene
 * and, with the ranges that travel in the program, on every context.
 * Declarations are not part of the encoding (`save` / `open` are unchanged); they are part of the name gen_to_image
 * keeps a scene's program under, values are not.  Indices are handed out in declaration order; declaring an id again
 * with the same range returns its index; the 65th parameter is MARAY_E_LIMIT; lo > hi or a NaN bound MARAY_E_ARG. */
uint64_t maray_var_id(const char *name);      /* the id `var(name)` makes */
int maray_scene_declare_param(maray_scene *s, uint64_t var_id, double lo, double hi, uint32_t *index /* may be NULL */);
int maray_scene_param_count(const maray_scene *s, uint32_t *n);
int maray_scene_param_info(const maray_scene *s, uint32_t index, uint64_t *var_id, double *lo, double *hi, double *value);   /* any may be NULL */
int maray_scene_set_param(maray_scene *s, uint32_t index, double value);      /* what gen / gen_to_image render with */
/* Shutter, the scene layer (host only; see "shutter" below): every declared parameter has a span s >= 0, finite, 0 until
 * set (else MARAY_E_ARG).  maray_scene_shutter_values writes the n x P matrix (frame-major; P = the declared count; n in
 * {1, 2, 4, 8, 16, 32, 64}, else MARAY_E_ARG) of the n frames' values around the scene's current values v: frame i of a
 * parameter with s > 0 is v + s * c_i, c_i = (2i + 1 - n) / (2n) -- exact in f64, then one multiply and one add, never
 * fused; the samples are centred on the plain render's value like spatial samples on its point.  A parameter with s == 0
 * has v itself in every frame, bit for bit (-0.0 and NaN included).  Spans, like values, are not part of a program's name. */
int maray_scene_set_param_span(maray_scene *s, uint32_t index, double span);
int maray_scene_param_span(const maray_scene *s, uint32_t index, double *span);
int maray_scene_shutter_values(const maray_scene *s, uint32_t n, double *out /* n * P doubles */);

/* ---- lowering: Expr -> tape ---------------------------------------------------
 * Replaces what the reference does per pixel in `Expr::eval2` + `Cache`
 * (src/lib.rs:623-670, src/cache.rs) with a one-time pass: fix_color, inline
 * Let/Var/Arc/Decor into one hash-consed DAG over R, G and B, fold constant
 * sub-trees with IEEE-exact ops only (never sin/exp/ln), hoist Y-only
 * sub-expressions into the ROW section, schedule, allocate value slots. */
typedef struct maray_tape maray_tape;

typedef struct maray_lower_opts {
    uint32_t hoist_rows;   /* 1 = hoist Y-only sub-expressions into the ROW section (default), 0 = off */
    uint32_t plain_cse;    /* 1 = hash-cons without commutative operand canonicalisation (reproduces the
                              op census of SURVEY.md §8(d)); 0 = canonicalise a+b/b+a etc. (default) */
    uint32_t no_fuse;      /* 1 = keep Step(Sin(a)) as two ops; 0 = fuse into MARAY_OP_STEPSIN (default) */
    uint32_t no_skips;     /* 1 = do not emit SKIPZ / SKIPNZ wave-level short circuits; 0 = emit them (default) */
    uint32_t no_row_guards; /* 1 = no row-level SKIPZ ops (guards that are y values: bounds of a boolean over a whole row) */
    uint32_t no_private_regions; /* 1 = row regions share hash-consed values with the rest of the tape (computed ahead of the
                              SKIP op, unconditionally); 0 = each row region re-derives the x-dependent values it reads (default) */
    uint32_t no_rebalance; /* 1 = keep chains of one boolean connective (max(t1, max(t2, ...))) as written; 0 = rebuild them as
                              balanced trees, whose sub-trees get row-level SKIP ops of their own (default) */
    uint32_t no_y_spans;   /* 1 = guards bound a boolean over a span of x on one row only (they read Y); 0 = guards monotone in y
                              too are bounded over the rows [YMIN, YMAX] as well, i.e. over a rectangle of pixels (default) */
} maray_lower_opts;

typedef struct maray_tape_info {
    uint32_t n_consts, n_row_ops, n_row_slots, n_yvals, n_pix_ops, n_pix_slots, n_app;
    /* algorithmic op counts (unique non-constant ops after hash-consing and
     * constant folding): total and by dependence class */
    uint32_t alg_ops, alg_ops_xy, alg_ops_x, alg_ops_y, alg_ops_uniform;
    uint32_t folded_ops;       /* constant ops folded on the host */
    uint32_t dag_nodes;        /* unique DAG nodes including leaves */
    uint32_t acc_operands;     /* operand reads served by ACC */
    uint32_t skip_ops;         /* SKIPZ / SKIPNZ ops in the PIXEL section */
    uint32_t bool_ops;         /* PIXEL ops whose value is provably +0.0 or 1.0 */
    uint32_t sin_ops, sin_bounded;   /* Sin/StepSin ops, and how many have a proven-bounded argument */
    uint32_t private_regions;  /* row regions that got private copies of the shared x-dependent values they read */
    uint32_t rebalanced_chains; /* boolean OR / AND chains rebuilt as balanced trees */
    uint32_t op_histogram[MARAY_OP_COUNT];   /* PIXEL section */
    uint32_t row_params[2];    /* bit p of the 64-bit mask {low, high word}: an op of the ROW section reads PARAM p.  The ROW outputs
                                * depend on these parameters' values only: a context keeps them while those are unchanged */
} maray_tape_info;

int maray_lower(const maray_scene *s, const maray_lower_opts *opts, maray_tape **out);
void maray_tape_free(maray_tape *t);
int maray_tape_program(const maray_tape *t, maray_program *out);   /* pointers valid until maray_tape_free */
int maray_tape_get_info(const maray_tape *t, maray_tape_info *out);
/* Parameters of the program: the scene's declared count when some op reads one, else 0 (then the program is the
 * version-2 one the scene always had); and the range that travels with it. */
int maray_tape_param_count(const maray_tape *t, uint32_t *n);
int maray_tape_param_range(const maray_tape *t, uint32_t index, double *lo, double *hi);
/* The program's REFINE section (include/maray_tape.h, maray_refine); n_ops = 0 when it has none.  Pointers valid until
 * maray_tape_free. */
int maray_tape_refine(const maray_tape *t, maray_refine *out);

/* ---- tape-level device ABI (what a Rust `RenderMethod::Hip` arm binds) --------
 * Replaces par_gen_to_image / wasm_par_gen_to_image (src/render.rs:35-192) and
 * the wasmer JIT (src/wasm.rs:136-158). */
typedef struct maray_ctx maray_ctx;

typedef struct maray_texture {   /* one `RgbImage` of textures::Textures (src/textures.rs:9-12) */
    const uint8_t *rgb;          /* interleaved RGB8, row-major, w*h*3 bytes */
    uint32_t w, h;
} maray_texture;

enum {
    MARAY_BACKEND_TAPE = 0,      /* tape interpreter kernel: tape + constants staged in LDS */
    MARAY_BACKEND_TAPE_SMEM = 1, /* tape interpreter kernel: tape streamed through the scalar cache */
    MARAY_BACKEND_JIT = 2,       /* tape specialised to straight-line HIP via hiprtc (GPU analogue of src/wasm.rs) */
    MARAY_BACKEND_AUTO = 3       /* the specialised kernels when their code objects are in the cache (MARAY_CACHE_DIR) or when
                                    building them (estimated from the tape's size) costs less than what they save over
                                    hint_mpixels of rendering; else the scalar-cache tape interpreter, which needs no build.
                                   (for a supersampling context hint_mpixels counts samples) */
};

typedef struct maray_ctx_opts {
    uint32_t backend;       /* MARAY_BACKEND_* */
    uint32_t hint_mpixels;  /* MARAY_BACKEND_AUTO: how many megapixels (2^20 pixels, rounded up) the caller is about to render with
                               this context; 0 = unknown / many.  The specialised kernels are worth their hiprtc build only
                               when that time is earned back (or when the code object cache already holds them). */
    uint32_t samples;       /* k x k samples per output pixel, k in {0, 1, 2, 4, 8} (0 = 1); see "supersampling" below */
    uint32_t filter;        /* MARAY_FILTER_*: how the k x k samples become pixels; see "reconstruction filter" below */
    uint32_t transfer;      /* MARAY_TRANSFER_* (offset 16): what the reduces (box, tent, shutter) average; see "transfer" below */
    uint32_t reserved[3];
} maray_ctx_opts;

/* ---- supersampling (anti-aliasing with an in-kernel box filter) ---------------------------------------------------
 * Supersampling is two steps.  maray_scene_supersample(s, k) (below) moves the scene onto a k x k finer grid, and a
 * context created with samples = k renders that program's raster in k x k blocks and writes only their means:
 *   - sample points: output pixel (px, py) has the samples x = px + (2i + 1 - k) / (2k), y = py + (2j + 1 - k) / (2k),
 *     i, j = 0 .. k-1 (centred on the point the plain render evaluates; exact in f64 for k a power of two);
 *   - each sample's channel is cast like a plain pixel (Rust `as u8`: saturating, NaN -> 0);
 *   - each output channel is the integer mean of its k^2 cast samples, rounding half up: (S + k^2/2) >> log2(k^2).
 *     An integer sum: the same result in any order, on any device split.
 * With samples = k every render entry point takes OUTPUT geometry (w, h, y0 / y1, blocks, tiles in output pixels and
 * rows; the program is evaluated at sample indices 0 .. k w - 1 and 0 .. k h - 1).  This is well-defined for any
 * program ("reduce the sample grid"); maray_gen_to_image with maray_gen_opts.samples pairs the two steps itself.
 * Limits: k outside {0, 1, 2, 4, 8}: MARAY_E_ARG; f64 planes with k > 1: MARAY_E_ARG; k w or k h above
 * MARAY_DOMAIN_MAX: MARAY_E_LIMIT.  Every back-end has a supersampling kernel (maray_tape_pixels_ss, maray_jit_pixels_ss);
 * AUTO chooses between them as for a plain render.  k = 0 or 1 is the plain render, unchanged. */
int maray_scene_supersample(maray_scene *s, uint32_t k);   /* X -> X/k - (k-1)/(2k), Y alike, size * k; k = 0 or 1: no change */

/* ---- reconstruction filter (what turns the samples of a supersampled render into pixels) ---------------------------
 * `filter` (maray_ctx_opts.filter, maray_gen_opts.filter) is MARAY_FILTER_BOX, the in-kernel mean described above and the
 * default, MARAY_FILTER_TENT, a tent (Bartlett) filter two output pixels wide whose footprint overlaps the neighbouring
 * pixels', or MARAY_FILTER_CATROM, a Catmull-Rom filter four pixels wide (after the tent, below).  TENT and CATROM both need
 * samples = k in {2, 4, 8}: either with samples 0 or 1 is MARAY_E_ARG, and so is any other filter value (2 among them).  A
 * TENT or CATROM context is created like a box one, from the SUPERSAMPLED program (maray_scene_supersample(s, k), then lower),
 * and every render entry point takes output geometry.  The tent:
 *   - s(a, b, c) is the cast (`as u8`) sample of channel c at integer sample index (a, b) of the k w x k h sample raster:
 *     what a plain context of the same program renders;
 *   - per axis the footprint of pixel p is the 2k sample indices k p + u, u = -k/2 .. 3k/2 - 1, with the integer weights
 *     t(u) = 2k - |2u + 1 - k| (k = 2: 1 3 3 1; k = 4: 1 3 5 7 7 5 3 1; k = 8: 1 3 .. 15 15 .. 3 1; their sum is 2 k^2);
 *   - indices are clamped to the IMAGE: a -> min(max(a, 0), k w - 1), b alike with k h - 1 -- never to a launch's rows, a
 *     band or a tile;
 *   - out(px, py, c) = (SUM_u SUM_v t(u) t(v) s(clamp(k px + u), clamp(k py + v), c) + W/2) >> log2 W, W = 4 k^4
 *     (64 / 1024 / 16384: a shift by 6 / 10 / 14).
 * All arithmetic is integer (a horizontal partial sum is <= 255 * 2 k^2 = 32640: 16 bits; the full sum <= 255 * 16384: 32
 * bits), so the picture is the same whatever the launch order, band size, tile cut or device split; a constant image comes
 * out unchanged, and every sample's weights over all pixels sum to the same value.
 * RGB8 only (f64 planes: MARAY_E_ARG); k w or k h above MARAY_DOMAIN_MAX: MARAY_E_LIMIT, as for box.
 * Output rows [y0, y1) read the sample rows [k y0 - k/2, k y1 + k/2) clipped to [0, k h): every entry point renders that halo
 * itself -- per row range, per row block, per host tile, per gen_to_image tile and worker.
 * How it runs: the context is a plain back-end (samples = 1; any of the three, AUTO chooses as for box) of the program behind
 * a wrapper that, per band of output rows, enqueues one ordinary launch of the band's sample rows plus halo into scratch of
 * the context and then maray_filter_tent<k> on the same stream.  The scratch grows to the largest call, is ordered by the
 * stream and freed with the context; the device-pointer forms return without a device synchronise.  A band holds about
 * 128 MiB of samples; MARAY_FILTER_BAND_ROWS=<output rows>, read when the context is created, overrides that (measurements,
 * tests).  maray_hip_ctx_set_params passes through; the shutter entry points average tent-filtered frames; maray_hip_time_rows
 * / _blocks time launches plus filter; maray_hip_kernel_name is the inner kernel's name + "+maray_filter_tent<k>".
 *
 * MARAY_FILTER_CATROM = 3 is the Catmull-Rom filter, the cubic BC-spline with B = 0, C = 1/2: four output pixels wide, with
 * negative lobes that keep edges sharp where box and tent only average.  The value 2 is unassigned and stays MARAY_E_ARG.
 * CATROM needs samples = k in {2, 4, 8} like TENT (0 or 1: MARAY_E_ARG), and CATROM together with MARAY_TRANSFER_SRGB is not
 * built: MARAY_E_ARG, reported before a device is looked for.  f64 planes and over-limit sizes are refused exactly as for TENT.
 * With s(a, b, c) as above:
 *   - per axis the footprint of pixel p is the 4k sample indices k p + u, u = -3k/2 .. 5k/2 - 1;
 *   - with n = |2u + 1 - k| (always odd, so never equal to D or 2D) and D = 2k the integer weights are
 *       e(u) =  3 n^3 - 5 n^2 D + 2 D^3             for n < D,
 *       e(u) = -  n^3 + 5 n^2 D - 8 n D^2 + 4 D^3   for D < n < 2D,
 *     which is 2 D^3 CatmullRom(n / D) exactly (k = 2: -3 -9 29 111 111 29 -9 -3).  Their sum per axis is 16 k^4 = 256 / 4096 /
 *     65536, a power of two; each residue class of u modulo k sums to 16 k^3 = 128 / 1024 / 8192 (the partition of unity: a
 *     constant image comes out unchanged); the extremes of e are 111 / -9, 987 / -75, 8115 / -605;
 *   - indices are clamped to the IMAGE, as for the tent -- never to a launch's rows, a band or a tile;
 *   - out(px, py, c) = min(max((SUM_u SUM_v e(u) e(v) s(clamp(k px + u), clamp(k py + v), c) + W/2) >> log2 W, 0), 255),
 *     W = (16 k^4)^2: a shift by 16 / 24 / 32.  The sum is signed and >> is an arithmetic shift; which way it rounds a
 *     negative sum cannot show, because every negative result is clamped to 0.
 * All arithmetic is integer, so the picture is the same whatever the launch order, band size, tile cut or device split.  The
 * widths, from the sums of the positive and of the negative weights (k = 2 / 4 / 8):
 *   - a horizontal partial sum lies in -6,120 .. 71,400 / -89,760 .. 1,134,240 / -1,403,520 .. 18,115,200: 26 bits signed
 *     at k = 8;
 *   - the full sum lies in -3,427,200 .. 20,138,880 / -798,504,960 .. 5,076,695,040 / -199,412,121,600 .. 1,294,628,782,080:
 *     25 / 33 / 41 bits of magnitude, one more with the sign.  At k = 4 and 8 a 32-bit accumulator is WRONG, signed or unsigned.
 * Output rows [y0, y1) read the sample rows [k y0 - 3k/2, k y1 + 3k/2) clipped to [0, k h): every entry point renders that
 * halo itself -- per row range, per row block, per host tile, per gen_to_image tile and worker.
 * How it runs: the tent's wrapper and bands (above) with that halo and maray_filter_catrom<k> in place of the tent's kernel:
 * 32-bit horizontal sums in LDS, 64-bit vertical sums at k = 4 and 8.  The band budget, MARAY_FILTER_BAND_ROWS, set_params,
 * the shutter entry points (a frame is the Catmull-Rom-filtered frame) and the timing entry points work as for the tent;
 * maray_hip_kernel_name is the inner kernel's name + "+maray_filter_catrom<k>". */
enum { MARAY_FILTER_BOX = 0, MARAY_FILTER_TENT = 1, MARAY_FILTER_CATROM = 3 };      /* (2 is unassigned: MARAY_E_ARG) */
/* The filter kernel on its own (measurements): average ms of one pass over a w x rows output image (k w x k rows samples in
 * scratch of the call's own, whatever they hold). */
int maray_hip_time_filter(int device, uint32_t w, uint32_t rows, uint32_t k, int reps, float *ms_avg);

/* ---- transfer (what the reduces average: encoded bytes, or light) ---------------------------------------------------
 * The RGB8 a context renders is shown as sRGB, so a mean of bytes is not a mean of light: a one-sample 0 / 255 checker
 * reduces to 128 where half the light is 188.  `transfer` (maray_ctx_opts.transfer, maray_gen_opts.transfer) is
 * MARAY_TRANSFER_NONE, the reduces described above and the default, or MARAY_TRANSFER_SRGB: every reduce -- box, tent,
 * shutter -- decodes its samples to 16-bit linear light, averages those and encodes the mean.  Any other value is MARAY_E_ARG,
 * reported before a device is looked for.  SRGB is defined by two tables, in integers throughout:
 *   - decode D[256], uint16: the 256 literals of include/maray_transfer_table.h (D[v] = floor(65535 lin(v / 255) + 0.5) with
 *     lin(c) = c / 12.92 for c <= 0.04045, else ((c + 0.055) / 1.055)^2.4; the literals are authoritative, not the formula).
 *     D[0] = 0, D[255] = 65535, strictly increasing, steps of 19 .. 583;
 *   - thresholds T[v] = (D[v - 1] + D[v] + 1) >> 1 for v = 1 .. 255 (T[0] = 0 in maray_transfer_table's output);
 *   - encode E(M) = the number of v in 1 .. 255 with T[v] <= M: the byte whose light is nearest to M, the upper one at a tie.
 *     E(D[v]) = v, so a constant region comes out unchanged.  T steps by at least 19: a 16-wide bin M >> 4 holds at most one
 *     threshold, which is what the kernels' 4096-entry encode table relies on.
 * Every reduce under SRGB computes out = E((SUM w_i D[s_i] + W/2) >> log2 W) with the samples s_i, weights w_i, footprints,
 * clamps and W of its NONE contract: box W = k^2; tent weights t(u) t(v), W = 4 k^4, indices clamped to the image; shutter
 * W = n.  All sums are integers, the largest the tent's at k = 8: 16384 * 65535 < 2^30, so the picture is the same for every
 * launch order, band, tile and device split.
 *   - a shutter call on a filtered SRGB context stays composable: frame i is exactly the RGB8 the context renders, and those
 *     bytes are decoded, averaged and encoded again;
 *   - with nothing to reduce (samples 0 or 1, no shutter call) an SRGB context renders exactly the plain bytes;
 *   - the SRGB reduces are RGB8 only: f64 planes are refused exactly where NONE refuses them (a samples <= 1 context still
 *     renders them);
 *   - the output is still plain RGB8: no sRGB / gAMA chunk is written to a PNG, and no other transfer curve exists.
 * How it runs: an SRGB context is a plain back-end (samples = 1; any of the three, AUTO chooses as ever) of the program behind
 * the wrapper the tent filter uses (above).  Box: per band one launch of sample rows [k y0, k y1) -- no halo -- and
 * maray_filter_box_lin<k>; the in-kernel box reduce is not used.  Tent: the band with its halo and maray_filter_tent_lin<k>
 * (32-bit horizontal sums: they need 24 bits).  Shutter: maray_shutter_reduce_lin per group of 8 frames, with 32-bit partial
 * sums between groups (64 * 65535 needs 22 bits): the context's shutter scratch is min(n, 8) F + (n > 8 ? 4 F : 0) bytes.
 * The kernels keep D and the encode table in LDS, filled once per block.  maray_hip_kernel_name is the inner kernel's name +
 * "+maray_filter_box_lin<k>" / "+maray_filter_tent_lin<k>" (samples <= 1: "+maray_shutter_reduce_lin"). */
enum { MARAY_TRANSFER_NONE = 0, MARAY_TRANSFER_SRGB = 1 };
/* The two tables of a transfer; needs no device.  NONE: the identity (decode[v] = thresholds[v] = v); SRGB: D and T as above,
 * thresholds[0] = 0.  Any other transfer, or a null pointer: MARAY_E_ARG. */
int maray_transfer_table(uint32_t transfer, uint16_t decode[256], uint16_t thresholds[256]);
/* maray_hip_time_filter for any reduce kernel: (CATROM, NONE) is maray_filter_catrom<k> (CATROM with SRGB: MARAY_E_ARG, not
 * built), (TENT, NONE) is maray_filter_tent<k>, (BOX, SRGB) maray_filter_box_lin<k>, (TENT,
 * SRGB) maray_filter_tent_lin<k>; (BOX, NONE) has no kernel of its own (the reduce is inside the pixel kernel): MARAY_E_ARG.
 * The measurement entry points fill their own sample buffers with one byte value, 0x5A; with MARAY_TIME_RANDOM_BYTES=1 in the
 * environment (read at each call) with pseudo-random bytes: for the SRGB kernels the best and the worst case of their LDS
 * tables (every read of a wavefront a broadcast; reads spread over all entries). */
int maray_hip_time_filter_ex(int device, uint32_t w, uint32_t rows, uint32_t k, uint32_t filter, uint32_t transfer, int reps, float *ms_avg);

int maray_hip_device_count(int *n);
/* Uploads tape, constants and textures to HBM once. */
int maray_hip_ctx_create(int device, const maray_program *prog, const maray_texture *tex, uint32_t n_tex,
                         const maray_ctx_opts *opts, maray_ctx **out);
void maray_hip_ctx_free(maray_ctx *c);
/* The values of the program's parameters for the launches enqueued AFTER this call (n = the program's count, else
 * MARAY_E_ARG; each value inside its range, else MARAY_E_ARG and every old value stays).  Returns without touching the
 * device: the next launch copies the values on its own stream in front of its ROW pass, from pinned staging, so the
 * device-pointer entry points still return without synchronising and several frames may be in flight.  Launches of one
 * context with different values go on one stream, or are ordered by the caller.  Every value is NaN until set. */
int maray_hip_ctx_set_params(maray_ctx *c, const double *values, uint32_t n);
int maray_hip_ctx_param_count(const maray_ctx *c, uint32_t *n);

/* Evaluate rows [y0, y1) of a w x h image: p = [x as f64, y as f64],
 * x in [0,w) (src/render.rs:88-95).  rgb8: (y1-y0)*w*3 bytes, interleaved RGB,
 * row-major, values cast like Rust `as u8` (saturating, NaN -> 0); rgb64:
 * (y1-y0)*w*3 doubles (the pre-cast f64 values), either may be NULL.
 * Host-pointer form (device -> host copy included). */
int maray_hip_render_rows(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1,
                          uint8_t *rgb8, double *rgb64);
/* Several row ranges ("tiles", rows [y0,y1) each, given as n_tiles pairs y0,y1), rendered in the given order into ONE
 * caller-owned RGB8 raster of the whole image (rgb8_image = first byte of image row 0; w*h*3 bytes).  This is what
 * one worker of a multi-GPU render calls for its share of the image (the host-side gather of SURVEY.md 8(e), the
 * collector thread of src/render.rs:54-83): tile k's device -> host copy runs under tile k+1's kernels, the call
 * joins at the end.  fn (may be NULL) is called on the calling thread after each tile's rows have landed.
 * A raster in pinned memory (maray_host_alloc / maray_host_register) is written by DMA directly at PCIe rate; a
 * pageable one is filled through a pinned staging ring of the context (an extra host copy). */
typedef void (*maray_tile_fn)(void *user, uint32_t y0, uint32_t y1);
int maray_hip_render_tiles(maray_ctx *c, uint32_t w, uint32_t h, const uint32_t *tiles_y0y1, uint32_t n_tiles,
                           uint8_t *rgb8_image, maray_tile_fn fn, void *user);
/* ---- shutter (motion blur: a temporal box filter averaged on the device) ------------------------------------------
 * A shutter render of n frames, n in {1, 2, 4, 8, 16, 32, 64} (else MARAY_E_ARG), takes `values`: an n x P matrix of
 * parameter values, frame-major, P = the program's parameter count (maray_hip_ctx_param_count).
 *   - frame i is exactly what the context renders in RGB8 after maray_hip_ctx_set_params(row i); on a samples = k context
 *     that is the box-filtered frame;
 *   - every output byte is (S + n/2) >> log2(n), S = the integer sum of that byte over the n frames (S <= 255 * 64: 16 bits
 *     hold it).  An integer mean: the same in any order;
 *   - RGB8 only: the shutter entry points take no f64 planes;
 *   - every value of every frame is checked against its declared range by maray_hip_ctx_set_params' rule before anything
 *     is enqueued: one bad value is MARAY_E_ARG, nothing is launched, nothing is written, the context's values stay;
 *   - the values maray_hip_ctx_set_params set are unchanged after the call (a plain render after a shutter render shows
 *     what it showed before), and a shutter call neither needs them nor counts as setting them: it is allowed on a context
 *     whose values were never set, and a plain render on that context is still refused;
 *   - n = 1 is the plain render with row 0; a program without parameters (P = 0) takes values = NULL, renders once and
 *     returns the plain picture for any n;
 *   - the device-pointer form enqueues everything on the caller's stream -- per frame the parameter copy and the ordinary
 *     launches, per group of 8 frames one pass of maray_shutter_reduce -- and returns without a device synchronise (past
 *     eight frames it may wait for its own earlier parameter copies); the host forms reduce each tile on the device and
 *     copy ONE raster to the host, not n;
 *   - scratch (frames and, above 8 frames, 16-bit partial sums) belongs to the context like its y-value and guard tables:
 *     ordered by the stream, grown to the largest call -- min(n, 8) F + (n > 8 ? 2 F : 0) bytes, F = the rows' RGB8 bytes
 *     + 16 rounded up to 256 -- and freed with the context.
 * check_rows / samples limits as for the plain entry points.  d_rgb8 may have any alignment. */
int maray_hip_render_rows_shutter(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, const double *values, uint32_t n,
                                  uint8_t *rgb8);
int maray_hip_render_rows_shutter_device(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, const double *values, uint32_t n,
                                         void *d_rgb8, void *stream);
int maray_hip_render_tiles_shutter(maray_ctx *c, uint32_t w, uint32_t h, const uint32_t *tiles_y0y1, uint32_t n_tiles,
                                   const double *values, uint32_t n, uint8_t *rgb8_image, maray_tile_fn fn, void *user);
/* The reduce on its own (measurements): average ms of the passes that reduce n >= 2 frames of `bytes` bytes in HBM. */
int maray_hip_time_shutter_reduce(int device, size_t bytes, uint32_t n, int reps, float *ms_avg);
/* The same with a transfer ("transfer" above): SRGB times the passes of maray_shutter_reduce_lin. */
int maray_hip_time_shutter_reduce_ex(int device, size_t bytes, uint32_t n, uint32_t transfer, int reps, float *ms_avg);
/* Pinned (page-locked, DMA-able from every device) host memory for output rasters: what backs the `RgbImage` a
 * caller hands to gen_to_image (src/lib.rs:1210) when it wants the PCIe rate.  maray_host_register pins memory the
 * caller already owns (e.g. a Rust Vec<u8>) for the time between the two calls. */
int maray_host_alloc(size_t bytes, void **out);
void maray_host_free(void *p);
int maray_host_register(void *p, size_t bytes);
int maray_host_unregister(void *p);
/* Device-pointer form: outputs stay in HBM; enqueued on `stream`
 * (a hipStream_t, NULL = the null stream); returns without synchronising. */
int maray_hip_render_rows_device(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1,
                                 void *d_rgb8, void *d_rgb64, void *stream);
/* Several row ranges in one launch: n_blocks blocks of block_rows consecutive rows, the first at y0, block_stride
 * rows apart (block_stride >= block_rows); outputs packed block after block.  This is how one rank of a multi-GPU
 * render takes its interleaved share of an image (blocks dealt round-robin, src/render.rs:35-99 deals rows the same
 * way to Rayon workers) without paying a launch per block. */
int maray_hip_render_blocks_device(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t block_rows, uint32_t block_stride,
                                   uint32_t n_blocks, void *d_rgb8, void *d_rgb64, void *stream);
/* Time `reps` launches of the pixel kernel for rows [y0,y1) with HIP events on
 * the launch stream; returns the average milliseconds per launch. */
int maray_hip_time_rows(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1,
                        void *d_rgb8, void *d_rgb64, int reps, float *ms_avg);
/* The same for the launch maray_hip_render_blocks_device issues (one rank's interleaved share of an image). */
int maray_hip_time_blocks(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t block_rows, uint32_t block_stride,
                          uint32_t n_blocks, void *d_rgb8, void *d_rgb64, int reps, float *ms_avg);
/* The part of a program's ROW section that y values [first_out, first_out + n_out) depend on, as the evaluators cut
 * it to run parts of the section side by side or per rectangle of pixels: a tape of its own (NOPs removed, SKIP
 * regions kept, value slots renumbered by liveness; *n_slots_out = slots it uses).  Free *ops_out with maray_free. */
int maray_row_cone(const maray_program *prog, uint32_t first_out, uint32_t n_out, uint64_t **ops_out, uint32_t *n_ops_out,
                   uint32_t *n_slots_out);
/* MARAY_BACKEND_JIT, offline: the HIP source generated for a tape (free with
 * maray_free) and the gfx950 code object hiprtc builds from it (needs no GPU). */
int maray_jit_source(const maray_program *prog, char **src_out);
/* ... and of the ROW kernel (one work-item per row; *n_chunks = how many independent chunks the
 * ROW section was cut into, evaluated side by side as blockIdx.y; may be NULL). */
int maray_jit_source_rows(const maray_program *prog, char **src_out, uint32_t *n_chunks);
int maray_jit_build(const maray_program *prog, void **code_out, size_t *len_out);
/* The supersampling PIXEL kernel (maray_jit_pixels_ss, k = 2, 4, 8: see "supersampling"): its source, and its gfx950 code
 * object (built once per program and k, kept like the others under a key of its own that contains k).  Needs no GPU.  The
 * plain sources above and their key do not depend on it. */
int maray_jit_source_samples(const maray_program *prog, uint32_t k, char **src_out);
int maray_jit_build_samples(const maray_program *prog, uint32_t k, void **code_out, size_t *len_out);
/* The specialised kernels of a program are built once and kept, in the process and under MARAY_CACHE_DIR (default
 * $XDG_CACHE_HOME/maray_amd or ~/.cache/maray_amd; "off" disables): the reference's JIT compiles its modules again on
 * every thread of every render (src/render.rs:158-165).  The key is a 128-bit hash of the generated sources, the
 * compiler options and the hiprtc version: 32 hex digits + NUL into out33.  Needs no GPU. */
int maray_jit_code_key(const maray_program *prog, char *out33);
int maray_jit_code_cached(const maray_program *prog, int *cached);
/* Name of the dominant kernel (for matching rocprofv3 rows). */
const char *maray_hip_kernel_name(const maray_ctx *c);
/* How many ROW passes (maray_jit_rows) and launch-order kernels (maray_jit_order) the context has enqueued since it was
 * created.  A MARAY_BACKEND_JIT context keeps a geometry's ROW outputs while the parameters the ROW section reads are
 * unchanged (MARAY_JIT_ROW_REUSE=0 in the environment when the context is created: a ROW pass per launch), so a launch
 * need not add to either; the interpreters' contexts report 0, 0. */
int maray_hip_launch_counts(const maray_ctx *c, uint64_t *row_passes, uint64_t *order_kernels);

/* ---- guard refinement (include/maray_tape.h, maray_refine) ----------------------------------------------------------
 * maray_hip_ctx_create with the program's REFINE section beside it (NULL, or n_ops = 0: exactly maray_hip_ctx_create).
 * A MARAY_BACKEND_JIT context then runs maray_jit_refine behind every ROW pass, on the same stream and into the same
 * guard words, in place: on the rectangles whose geometric bit is set it evaluates the section and clears the bits it
 * proves zero.  The words belong to the set of ROW outputs the pass filled, so the refinement is kept, reused and
 * dropped with them.  MARAY_JIT_GUARD_REFINE=0 in the environment when the context is created: no such launch (rasters
 * are identical either way; not part of a code key).  The interpreters ignore the section. */
int maray_hip_ctx_create_refined(int device, const maray_program *prog, const maray_refine *refine, const maray_texture *tex, uint32_t n_tex,
                                 const maray_ctx_opts *opts, maray_ctx **out);
/* Source of maray_jit_refine for a program and its REFINE section (free with maray_free); the empty string when the
 * section gives no kernel (no section, or no guard words).  Needs no GPU. */
int maray_jit_source_refine(const maray_program *prog, const maray_refine *refine, char **src_out);
/* ... and its gfx950 code object (free with maray_free; *len_out = 0 when there is no kernel), built once and kept like
 * the other modules', under a key of its own made of its text.  Needs no GPU. */
int maray_jit_build_refine(const maray_program *prog, const maray_refine *refine, void **code_out, size_t *len_out);
/* Test access: how MARAY_BACKEND_JIT keeps the program's guards.  pos[g] = the bit of guard g (y value n_yvals - *n_guards + g)
 * in a rectangle's words, -1 for a guard derived from other guards' bits (at most `cap` entries are written); *n_words =
 * 64-bit words per rectangle (0: the guards are not kept as bits), *gw x *gh = the rectangle in pixels x rows.  Needs no GPU. */
int maray_jit_guard_layout(const maray_program *prog, int32_t *pos, uint32_t cap, uint32_t *n_guards, uint32_t *n_words, uint32_t *gw, uint32_t *gh);
/* The census of guard bits (MARAY_BACKEND_JIT, plain contexts that reuse their ROW outputs).  The first launch that finds a
 * set of ROW outputs filled runs maray_jit_census over the set's geometry -- the PIXEL kernel's own text without its stores,
 * recording per rectangle which guarded shapes are != 0 on some pixel -- and maray_jit_census_apply, which writes the set's
 * words without the eligible guard bits of the others into a second table of the set, which that launch and the later ones of
 * the set read (the ROW pass's words stay what they are); then the launch order, then the pixels.  Once per filling of a set;
 * a launch of more than 65,534 rows takes none.  MARAY_JIT_GUARD_CENSUS=0 in the environment when the context is created: no
 * such launch (rasters are identical either way; not part of a code key).
 * maray_hip_census_count: how many the context has enqueued (0 for an interpreter's context).
 * maray_jit_census_eligible: per guard word of a rectangle (see maray_jit_guard_layout), the bits a census may clear: bits of
 * leaves of a guarded reduction of the PIXEL section that gate nothing else, read no parameter the ROW section does not read
 * and hold no Sin that may send its tile to the interpreter; at most `cap` words are written, *n_words = words per rectangle.
 * maray_jit_source_census: the kernels' source ("" when no bit is eligible; free with maray_free).  Neither needs a GPU. */
int maray_hip_census_count(const maray_ctx *c, uint64_t *census_launches);
int maray_jit_census_eligible(const maray_program *prog, uint64_t *mask, uint32_t cap, uint32_t *n_words);
int maray_jit_source_census(const maray_program *prog, char **src_out);
/* How many maray_jit_refine passes the context has enqueued since it was created (0 for an interpreter's context). */
int maray_hip_refine_count(const maray_ctx *c, uint64_t *refine_passes);
/* Test access: the guard words of the set of ROW outputs the most recent launch used, copied to the host after everything
 * enqueued on the context so far has completed.  *n_words = words in the set (rectangles x words per rectangle, the
 * rectangles of a group of rows adjacent), *words_per_rect = words per rectangle; at most `cap` words are copied.
 * MARAY_E_ARG for a context without guard words or before its first launch. */
int maray_hip_debug_guard_words(maray_ctx *c, uint64_t *words, size_t cap, size_t *n_words, uint32_t *words_per_rect);
/* The same for the words the most recent launch READ: those of maray_hip_debug_guard_words, which the ROW pass and the second
 * bounds wrote, until the set has been through its census; from then on what maray_jit_census_apply left of them. */
int maray_hip_debug_census_words(maray_ctx *c, uint64_t *words, size_t cap, size_t *n_words, uint32_t *words_per_rect);
/* The cover of guarded ORs (MARAY_BACKEND_JIT, wherever a census is taken).  A boolean OR of guarded shapes that the census may
 * decide gets a cover bit: a bit of the last guard word that no guard uses (never a word more; a program without free bits
 * gets none).  Behind a set's census maray_jit_cover -- the PIXEL kernel's text without its stores, over the census'd words --
 * records per rectangle whether the OR of the shapes that read no parameter the ROW section does not read and hold no Sin that
 * may defer its tile is 1 on every pixel inside the picture; maray_jit_cover_apply writes a third table of words in which such
 * a rectangle has its cover bit set and those of the OR's eligible guard bits cleared that no other reduction has a leaf on.  A set with at least one cover bit is rendered by
 * maray_jit_pixels_cov, maray_jit_pixels with one scalar test per such OR: bit set, the OR is all-ones and no shape is entered.
 * Once per filling of a set, like the census.  MARAY_JIT_GUARD_COVER=0 in the environment when the context is created: none of
 * it (rasters are identical either way; not part of a code key).
 * maray_hip_cover_count: maray_jit_cover launches the context has enqueued.
 * maray_jit_cover_bits: the plan as int32 values: n, then per OR with a bit: its bit, its root op, its number of guarded
 * leaves, and per leaf: its last op, its guard bit, 1 if the measurement leaves it out (tainted), 1 if its bit is cleared under
 * a cover bit (census-eligible).  At most `cap` values are written, *n_values = how many there are.
 * maray_jit_source_cover: the three kernels' source ("" when the program gets no bit; free with maray_free).
 * maray_hip_debug_cover_words: like maray_hip_debug_census_words; the third table where the most recent launch read it.
 * maray_jit_cover_bits and maray_jit_source_cover need no GPU. */
int maray_hip_cover_count(const maray_ctx *c, uint64_t *cover_launches);
int maray_jit_cover_bits(const maray_program *prog, int32_t *values, uint32_t cap, uint32_t *n_values);
int maray_jit_source_cover(const maray_program *prog, char **src_out);
int maray_hip_debug_cover_words(maray_ctx *c, uint64_t *words, size_t cap, size_t *n_words, uint32_t *words_per_rect);
/* Row words (MARAY_BACKEND_JIT, wherever a cover is taken -- or a census, for a program without cover bits -- for programs with
 * up to 12 guard words and rectangles of 64 pixels, and launches whose guard groups are more than one row high).  Behind a
 * set's cover maray_jit_rowscan forms the words of every (rectangle, row): the band's, without the census-eligible bits of
 * leaves that are 0 on that row and with the cover bits of the ORs whose untainted leaves cover it.  maray_jit_rowscan_apply sets
 * the ROW FLAG, one more free bit of the last guard word (a program without one gets no row words), in a fourth table for the
 * rectangles where at least a quarter of the band's rows differ from the band.  A set with at least one flag is rendered by
 * maray_jit_pixels_rw: maray_jit_pixels_cov, whose flagged rectangles take their words of the row at hand.  The module is built
 * by the first launch that is due a scan (which waits for it), never when a context is created.  The tables count against the
 * kept sets' budget; a set they do not fit takes none.  MARAY_JIT_ROW_WORDS=0 in the environment when the context is created:
 * none of it (rasters are identical either way; not part of a code key).
 * maray_hip_rowscan_count: maray_jit_rowscan launches the context has enqueued.
 * maray_jit_rowwords_flag: the row flag's bit, -1 when the program gets no row words.  maray_jit_source_rowwords: the two
 * kernels' source ("" when it gets none; free with maray_free).  Neither needs a GPU.
 * maray_hip_debug_row_words (test access): of the set the most recent launch used, the fourth table (like
 * maray_hip_debug_cover_words) and the row words, n_gwords per (row of the call, rectangle); *n_xbits = *n_rwords = 0 for a set
 * that has been through no scan; *used = 1 when that launch ran maray_jit_pixels_rw.
 * maray_hip_debug_row_sets (test access): the kept sets of ROW tables of a MARAY_BACKEND_JIT context: the set the most recent
 * launch used (0 = the scratch, -1 before any launch), how many sets are kept, the bytes accounted to them, their budget
 * (MARAY_ROW_KEPT_BYTES), and the device bytes the kept sets' tables hold (every table's capacity times its element size).
 * Host state only: it waits for nothing and changes nothing.  MARAY_E_ARG for an interpreter's context. */
int maray_hip_rowscan_count(const maray_ctx *c, uint64_t *rowscan_launches);
int maray_jit_rowwords_flag(const maray_program *prog, int32_t *flag_bit);
int maray_jit_source_rowwords(const maray_program *prog, char **src_out);
int maray_hip_debug_row_words(maray_ctx *c, uint64_t *xbits, size_t xcap, size_t *n_xbits, uint64_t *rwords, size_t rcap, size_t *n_rwords,
                              uint32_t *words_per_rect, int *used);
/* The pre-pass (MARAY_BACKEND_JIT, for the programs that get row words): maray_jit_pixels_pp is maray_jit_pixels_rw with one
 * addition on the fast RGB8 path.  A rectangle whose guard words -- of the row at hand, where it has row words -- are zero
 * apart from cover bits has no shape-dependent pixel; a busy tile with such a rectangle renders those in one pass four pixels
 * per lane and runs its narrow passes over the other rectangles only.  The module is built beside the row-word module by the
 * launch that builds that one; where it is in place it renders every set that maray_jit_pixels_cov or maray_jit_pixels_rw
 * rendered.  MARAY_JIT_PREPASS=0 in the environment when the context is created: none of it (rasters are identical either
 * way; not part of a code key).
 * maray_hip_prepass_count: launches of maray_jit_pixels_pp the context has enqueued.  maray_jit_source_prepass: the kernel's
 * source ("" when the program gets none; free with maray_free); needs no GPU.
 * maray_hip_deferred_count (test access): the 256-pixel tiles the most recent launch of a MARAY_BACKEND_JIT context handed to
 * the interpreter (a Sin whose argument is huge); waits for the context's work.  0 for other contexts. */
int maray_hip_deferred_count(maray_ctx *c, uint64_t *deferred_tiles);
int maray_hip_prepass_count(const maray_ctx *c, uint64_t *prepass_launches);
int maray_jit_source_prepass(const maray_program *prog, char **src_out);
int maray_hip_debug_row_sets(const maray_ctx *c, int32_t *set, uint32_t *kept_sets, uint64_t *kept_bytes, uint64_t *budget_bytes, uint64_t *held_bytes);

/* ---- render façade: gen_to_image / gen (src/lib.rs:1177-1213) -----------------*/
enum {                         /* RenderMethod (src/lib.rs:1155-1173), extended */
    MARAY_METHOD_HIP = 3       /* 0..2 are the reference's CPU methods, not provided here */
};
enum { MARAY_REPORT_NONE = 0, MARAY_REPORT_ROW = 1, MARAY_REPORT_DURATION_MS = 2 };   /* Report (src/report.rs:17-24) */

typedef struct maray_report {
    uint32_t kind;    /* MARAY_REPORT_* */
    uint32_t value;   /* rows, or milliseconds */
} maray_report;

/* F: Fn(&mut RgbImage, f64) (src/lib.rs:1185): image so far + progress y/h.
 * Invoked on the calling thread between row tiles. */
typedef void (*maray_report_fn)(void *user, uint8_t *rgb8, uint32_t w, uint32_t h, double progress);

typedef struct maray_gen_opts {
    uint32_t backend;        /* MARAY_BACKEND_* */
    uint32_t n_devices;      /* 0 = all visible devices; image rows are tiled across them */
    uint32_t tile_rows;      /* rows per launch (0 = default) */
    uint32_t samples;        /* k x k samples per pixel (0 = 1): the scene is supersampled privately and rendered by
                                contexts with samples = k; programs are kept per k */
    uint32_t shutter;        /* n frames averaged over the scene's parameter spans (maray_scene_shutter_values; n in {0, 1, 2, 4,
                                ..., 64}).  0, 1 or no span above 0: the plain render, exactly.  The program and its contexts are
                                the plain render's: spans and n are not part of their name */
    uint32_t filter;         /* MARAY_FILTER_* ("reconstruction filter"); TENT and CATROM need samples in {2, 4, 8}; programs and contexts
                                are kept per (k, filter) */
    uint32_t encoder;        /* MARAY_ENCODER_* (offset 24): who writes maray_gen's PNG; see "device PNG encoder" below.  Any other value:
                                MARAY_E_ARG.  maray_gen_to_image checks the word and otherwise ignores it */
    uint32_t transfer;       /* MARAY_TRANSFER_* (offset 28; "transfer"): programs and contexts are kept per (k, filter, transfer) */
} maray_gen_opts;
enum { MARAY_ENCODER_HOST = 0, MARAY_ENCODER_DEVICE = 1 };
/* A flag on `encoder`: the device encoder with dynamic-Huffman codes ("device PNG encoder": MARAY_PNG_CODES_DYNAMIC).  The
 * valid words are 0, 1 and MARAY_ENCODER_DEVICE | MARAY_ENCODER_DYNAMIC; the flag alone is MARAY_E_ARG like every other word. */
#define MARAY_ENCODER_DYNAMIC 0x100

/* gen_to_image: fills the caller's w*h*3 RGB8 buffer. */
int maray_gen_to_image(const maray_scene *s, const maray_texture *tex, uint32_t n_tex,
                       const maray_gen_opts *opts, maray_report report, maray_report_fn fn, void *user,
                       uint8_t *rgb8, uint32_t w, uint32_t h);
/* gen_to_image keeps what a call sets up -- the scene's tape and one context per device -- for the next call with the
 * same scene, textures and back-end (the last MARAY_GEN_CACHE programs, default 4, 0 = none): an animation that calls
 * it in a loop (examples/test*.rs) pays the lowering and the context creation once, not per frame.  This frees them. */
void maray_gen_cache_clear(void);
/* What is kept, one line per idle context: "<program key> device <d> kernel <name> hint_mpixels <n>" (NUL-terminated,
 * cut to cap; " samples <k>" follows for k > 1, " filter tent" / " filter catrom" after that for MARAY_FILTER_TENT /
 * MARAY_FILTER_CATROM and " transfer srgb" last for MARAY_TRANSFER_SRGB).  Under MARAY_BACKEND_AUTO a kept interpreter context is replaced when a later call renders more than
 * the call it was chosen for; contexts are kept per physical device. */
int maray_gen_cache_info(char *out, size_t cap);
/* gen: render and write a PNG (progress callback prints "%.2f %%" to stderr
 * and re-saves the partial image, like src/lib.rs:1203-1208).
 * With opts->encoder = MARAY_ENCODER_DEVICE every worker renders its tiles with maray_hip_render_rows_device (or, for a shutter
 * call, maray_hip_render_rows_shutter_device) into its encoder's band buffer, encodes them on its own device and hands over
 * only the compressed segments; the calling thread puts the file together in row order (the same bytes for any n_devices and
 * tile_rows).  With a report the percentage is still printed, but the partial file is NOT re-saved: there is no host raster.
 * A scene of size 0 in x or y is MARAY_E_ARG with this encoder.  With MARAY_ENCODER_DEVICE | MARAY_ENCODER_DYNAMIC every worker's
 * encoder writes dynamic codes: the same pixels in a smaller file, whose bytes depend on n_devices and tile_rows. */
int maray_gen(const maray_scene *s, const maray_texture *tex, uint32_t n_tex,
              const maray_gen_opts *opts, maray_report report, const char *png_path);

/* ---- device PNG encoder ------------------------------------------------------------------------------------------
 * MARAY_ENCODER_DEVICE builds the zlib stream of the PNG on the device: the compressed stream crosses to the host, not the
 * raster, and the host's zlib compression goes away.  PNG container bytes are an encoder's choice: the file decodes to the
 * same RGB8 raster as the host writer's (maray_png_write: filter 0, zlib level 6, the default, unchanged), not to the same
 * bytes.  The result is an ordinary PNG -- IHDR (8-bit truecolour, no interlace), IDAT chunks of at most 2^30 bytes, IEND,
 * CRC-32 by zlib's crc32 -- around this stream:
 *   - filtered data: row y is one filter byte followed by the row's 3 w bytes.  The encoder writes filter 0 (None) in every
 *     row unless a row filter is asked for ("Row filters" below: any type 0 .. 4);
 *   - segments: each row's 3 w + 1 filtered bytes are cut into segments of SEG = 256 pixels (the last of a row may be
 *     shorter; the filter byte belongs to the row's first segment).  Segments are compressed independently: no match
 *     reaches back over a segment's start;
 *   - a segment is whole deflate blocks followed by an empty stored block that ends on a byte boundary: the 3 bits BFINAL = 0,
 *     BTYPE = 00, zero bits to the byte, then 00 00 FF FF (the sync flush pigz uses);
 *   - the stream is 78 01, the segments in row-major order, 01 00 00 FF FF (a final empty stored block), and the Adler-32 of
 *     all filtered bytes, big-endian;
 *   - the file's bytes are therefore a function of the raster alone: identical for every band height (MARAY_PNG_BAND_ROWS),
 *     tile cut, stream and device split;
 *   - coding: one fixed-Huffman block (BTYPE = 01) per segment.  Literals are the standard fixed codes; a run of pixels equal
 *     to the pixel before them is coded as matches of distance 3 (distance code 2, no extra bits) whose length is a multiple
 *     of 3 and at most 258 (here: at most 192, a run is closed every 64 pixels); Huffman codes go into the LSB-first bit
 *     stream bit-reversed, extra bits as they are;
 *   - Adler-32: per segment of n bytes b_0 .. b_(n-1) the device forms A = sum b_i and B = sum (n - i) b_i; from (s1, s2) =
 *     (1, 0) the segments in order give s2 <- (s2 + n s1 + B) mod 65521, then s1 <- (s1 + A) mod 65521.  The device combines a
 *     band's segments -- a run of segments is again such a triple (n, A, B), and a segment's share of its band's B is
 *     B + A x (the band's bytes after the segment), so the shares add up in any order -- and three words modulo 65521 per
 *     band come to the host, which combines the bands in order.  The raster never reaches the host;
 *   - size: a segment of n bytes occupies at most ceil(9 n / 8) + 16 bytes (9-bit literals, block header, end-of-block, sync):
 *     that is its scratch slot.  There is no stored-block fallback.
 * How it runs: per band of rows (64 MiB of raster; MARAY_PNG_BAND_ROWS=<rows>, read when an encoder is created, overrides
 * that) maray_png_compress (one wavefront per segment), maray_png_scan (offsets of the segments, the band's Adler part) and
 * maray_png_gather (the contiguous stream) on one stream; then one copy of 24 bytes (the total and the Adler part) and one of
 * exactly the stream's bytes into pinned staging.  Scratch -- slots, lengths, offsets, the gathered stream, a band buffer for
 * the entry points that render -- belongs to an encoder, grows to the largest call and is freed with it; the library keeps
 * up to two idle encoders per device.  All sizes and offsets past a band are 64-bit.
 * Errors: a null pointer, w = 0 or h = 0: MARAY_E_ARG; a side above MARAY_DOMAIN_MAX or (3 w + 1) h above 2^34 (the host
 * writer's limit): MARAY_E_LIMIT; nothing is launched in those cases. */
/* A packed RGB8 raster in device memory (any byte alignment) -> a complete PNG in malloc'ed host memory (maray_free).  The
 * kernels and copies are enqueued on `stream` (a hipStream_t, NULL = the null stream); the call waits for them, and for
 * nothing else. */
int maray_hip_png_encode_device(int device, const void *d_rgb8, uint32_t w, uint32_t h, void *stream, uint8_t **png_out, size_t *n_out);
/* The whole w x h image of a context (any back-end, samples, filter) as a PNG: rendered band by band through the device
 * entry points into the encoder's band buffer and encoded there; no raster crosses to the host.  values = NULL: the plain
 * render (maray_hip_render_rows_device); else a shutter call of n_frames frames (maray_hip_render_rows_shutter_device, same
 * checks, nothing launched when one fails). */
int maray_hip_render_png(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, uint8_t **png_out, size_t *n_out);
/* Measurements: average ms of the three kernels over the caller's raster as ONE band ((3 w + 1) h <= 2^30), and the bytes
 * of its gathered stream; and the bytes the process' encoders have copied to the host so far (payloads and totals). */
int maray_hip_time_png_encode(int device, const void *d_rgb8, uint32_t w, uint32_t h, int reps, float *ms_avg, uint64_t *stream_bytes);
uint64_t maray_hip_png_bytes_to_host(void);
/* Dynamic-Huffman codes: a second way of coding the SAME tokens, opt-in everywhere; MARAY_PNG_CODES_FIXED is everything
 * above, byte for byte.  Any other value of a `codes` argument: MARAY_E_ARG, reported before a device is looked for.
 *   - tokens: exactly the fixed coder's.  Each row is one filter byte 0 plus 3 w bytes, cut into segments of SEG = 256
 *     pixels; a segment's first pixel is literal; a run of pixels equal to the pixel before them is one match of distance 3
 *     whose length is a multiple of 3 and at most 192 (a run is closed at every 64-pixel step).  The token sequence is a
 *     function of the raster alone; only the codes differ;
 *   - a band's piece: per band of rows the device counts the tokens, the host fits a code to the counts, and the device
 *     writes the band as ONE dynamic block: BFINAL = 0, BTYPE = 10; HLIT, HDIST, HCLEN, the code-length code and the
 *     lengths (the run symbols 16 .. 18 may be used or not: today they are not); every segment's tokens in row-major order
 *     with nothing between segments; symbol 256; then the empty stored block that ends on a byte boundary (three zero bits,
 *     zeros to the byte, 00 00 FF FF).  Pieces concatenate at byte granularity, and the stream around them is unchanged:
 *     78 01, the pieces, 01 00 00 FF FF, the Adler-32;
 *   - codes: any prefix code with lengths of at most 15 in which length 0 is given to exactly the unused symbols and the
 *     literal/length code is complete (symbols 0 and 256 always occur: it has at least two symbols).  The distance code set
 *     is the symbols 0, 1, 2 with lengths 0 0 1 when the band holds a match, and one symbol of length 0 when it holds none.
 *     Where the unrestricted Huffman tree of the band's counts is at most 15 deep the code costs what that tree costs (an
 *     optimal code; the cost is unique though the tree is not); deeper, it is an optimal code among those of at most 15 bits;
 *   - what the bytes depend on: the raster AND how its rows were cut into bands and encode calls (MARAY_PNG_BAND_ROWS,
 *     tile_rows, the device split) -- unlike the fixed coder's "function of the raster alone".  The decoded raster does not
 *     depend on the cut; the same raster and the same cuts give the same bytes on every stream and in every run;
 *   - band size: a dynamic band holds at most 2^28 filtered bytes (MARAY_PNG_BAND_ROWS is clipped to that), so every bit
 *     offset inside a band is below 15 x 2^28 < 2^32; everything past a band is 64-bit, as above;
 *   - slot: a segment of n bytes takes at most ceil(15 n / 8) bytes of scratch;
 *   - errors, limits and the Adler-32: unchanged.
 * How it runs, per band: maray_png_histogram (the compress kernel's tokeniser feeding 286 counts in LDS; a capped grid that
 * strides over the segments; every block stores its partial counts) and maray_png_histogram_sum; 1,152 bytes of counts to the
 * host, which fits the code (maray_png_dynamic_codes) and sends back 1,144 bytes of codes; maray_png_compress_dyn (a
 * segment's bits into its slot, its length in bits), maray_png_scan (bit offsets), maray_png_zero and maray_png_gather_bits
 * (every segment's bits shifted to its place behind the header's); then the totals and exactly the piece's bytes. */
enum { MARAY_PNG_CODES_FIXED = 0, MARAY_PNG_CODES_DYNAMIC = 1 };
/* The three entry points above with a `codes` argument; with MARAY_PNG_CODES_FIXED each is exactly the call it extends. */
int maray_hip_png_encode_device_ex(int device, const void *d_rgb8, uint32_t w, uint32_t h, uint32_t codes, void *stream, uint8_t **png_out,
                                   size_t *n_out);
int maray_hip_render_png_ex(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, uint32_t codes, uint8_t **png_out,
                            size_t *n_out);
/* (DYNAMIC: ONE band is (3 w + 1) h <= 2^28; the band's code is fitted once, before the timed loop; the kernels timed are the
 * six above, and *stream_bytes the bytes of the band's piece) */
int maray_hip_time_png_encode_ex(int device, const void *d_rgb8, uint32_t w, uint32_t h, uint32_t codes, int reps, float *ms_avg,
                                 uint64_t *stream_bytes);
/* The host's part on its own; needs no device.  From a band's counts -- lit_counts[256] >= 1 and at least one more symbol;
 * of the distance counts only dist_counts[2] may be above 0 (else MARAY_E_ARG) -- the code lengths, and in `header` the
 * block's bits LSB-first from BFINAL up to but not including the first token (*header_bits of them, at most 2,286; the rest
 * of the last byte is zero).  cap < ceil(*header_bits / 8): MARAY_E_ARG. */
int maray_png_dynamic_codes(const uint32_t lit_counts[286], const uint32_t dist_counts[30], uint8_t lit_lens[286], uint8_t dist_lens[30],
                            uint8_t *header, size_t cap, size_t *header_bits);
/* Row filters: the filter byte of every row, opt-in everywhere; MARAY_PNG_FILTER_NONE is everything above, byte for byte.
 * A filter turns a vertical repeat or a ramp into a constant, and a constant is what the distance-3 run tokeniser codes well.
 *   - the option: NONE writes type 0 in every row; SUB .. PAETH force PNG type 1 .. 4 on every row (each filter's arithmetic
 *     on its own); ADAPTIVE picks a type per row by the rule below.  Any other value: MARAY_E_ARG, reported before a device
 *     is looked for;
 *   - arithmetic: PNG's, with bpp = 3, over the WHOLE row -- segments cut the compression, not the filter: the left and
 *     upper-left neighbours of a segment's first pixel are the previous segment's last pixels; neighbours left of x = 0 are 0,
 *     and so is the row above row 0; Average is floor((a + b) / 2) on the 9-bit sum; Paeth breaks ties in the order a, b, c;
 *     everything modulo 256;
 *   - tokens: the tokeniser above, applied to the FILTERED pixels: a segment's first pixel is literal, a run of filtered
 *     pixels equal to the filtered pixel before them is one distance-3 match, closed every 64 pixels; the filter byte t is the
 *     literal in front of the row's first segment.  The slot bounds hold for any bytes: unchanged.  The Adler-32 is over the
 *     filtered bytes, t included;
 *   - the rule (ADAPTIVE), exact integer arithmetic and independent of launch order: for row y and type t, bytes_t = the sum
 *     over the row's segments of the bytes the segment occupies as a fixed-Huffman segment under t, bits_t = the sum of those
 *     segments' token bits (block header, filter byte and tokens, without the end-of-block); the row takes the smallest
 *     (bytes_t, bits_t, t).  With dynamic codes the SAME rule with the fixed codes' costs is used: a proxy, not that coder's
 *     own optimum;
 *   - size: with fixed codes a row's ADAPTIVE bytes are never more than its type-0 bytes, so an ADAPTIVE file is never larger
 *     than the NONE file of the same raster.  Forced types promise nothing;
 *   - the row above a cut: a band's first row is filtered like any other row (later bands of a raster read the row above
 *     them in the raster; maray_hip_render_png_opts keeps a band's last row in a 3 w-byte carry buffer, copied on the stream
 *     before the next band is rendered).  With fixed codes the file therefore stays a function of the raster and the filter
 *     option alone: the same for every MARAY_PNG_BAND_ROWS and stream.  With dynamic codes the bytes depend on the cut as
 *     above; the filter types and the decoded raster do not;
 *   - maray_gen and the animations (maray_gen_animation, maray_hip_render_apng, maray_hip_apng_encode_device) do not take the
 *     option: maray_gen_opts.encoder has no word for it.
 * How it runs, per band, before the kernels above: ADAPTIVE: maray_png_filter_cost (one wavefront per segment: the tokeniser's
 * counting for all five types at once, five (bytes, bits) pairs per segment) and maray_png_filter_pick (one wavefront per
 * row); a forced type: the rows' types are set to the constant.  Then the filtered forms of maray_png_compress,
 * maray_png_histogram and maray_png_compress_dyn read the row's type. */
enum { MARAY_PNG_FILTER_NONE = 0, MARAY_PNG_FILTER_ADAPTIVE = 1, MARAY_PNG_FILTER_SUB = 2, MARAY_PNG_FILTER_UP = 3, MARAY_PNG_FILTER_AVERAGE = 4, MARAY_PNG_FILTER_PAETH = 5 };
/* The encoder's options: `codes` (MARAY_PNG_CODES_*), `filter` (MARAY_PNG_FILTER_*), and six reserved words that must be 0
 * (else MARAY_E_ARG).  A null pointer stands for all zeros. */
typedef struct { uint32_t codes, filter, reserved[6]; } maray_png_opts;
/* The three entry points with the options; with filter = MARAY_PNG_FILTER_NONE each is exactly its `_ex` form. */
int maray_hip_png_encode_device_opts(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_opts *opts, void *stream,
                                     uint8_t **png_out, size_t *n_out);
int maray_hip_render_png_opts(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, const maray_png_opts *opts,
                              uint8_t **png_out, size_t *n_out);
/* (with a filter the kernels timed include maray_png_filter_cost and maray_png_filter_pick, or the constant's fill) */
int maray_hip_time_png_encode_opts(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_opts *opts, int reps, float *ms_avg,
                                   uint64_t *stream_bytes);

/* Indexed colour: PNG colour type 3 for rasters of at most 256 colours, opt-in through a family of its own (maray_png_opts
 * cannot grow); MARAY_PNG_COLOR_RGB is everything above, byte for byte.  Everything not named here is the truecolour contract
 * unchanged: 78 01, segments in row-major order, one fixed-Huffman block per segment followed by the empty stored block that
 * ends on a byte boundary, 01 00 00 FF FF, the Adler-32, IDAT chunks of at most 2^30 bytes, CRCs, the size checks.
 *   - palette: the n <= 256 distinct colours of the WHOLE raster, ascending by R * 65536 + G * 256 + B; a pixel's index is its
 *     colour's position in that order.  PLTE holds exactly n entries; there is no tRNS; chunk order IHDR, PLTE, IDAT.., IEND;
 *   - bit depth: d = 1 for n <= 2, 2 for n <= 4, 4 for n <= 16, else 8 (the smallest PNG allows); IHDR says depth d, colour
 *     type 3, no interlace;
 *   - filtered data: row y is one filter byte 0 followed by rb = ceil(w d / 8) packed bytes, the leftmost pixel in the
 *     high-order bits, the unused low bits of a row's last byte zero;
 *   - segments: a row's packed bytes are cut into segments of 768 bytes (the last of a row may be shorter); the filter byte
 *     belongs to the row's first segment, so a segment is at most 769 bytes, the truecolour maximum, and the slot bound
 *     ceil(9 n / 8) + 16 carries over.  Segments are compressed independently;
 *   - tokens: the filter byte is a literal, a segment's first packed byte is a literal.  The packed bytes of a segment are
 *     taken in steps of 64.  A byte equal to the byte before it IN THE SAME SEGMENT is "repeated" (the first byte of a later
 *     step is compared with the last byte of the step before).  A maximal run of L repeated bytes inside one step (a run is
 *     closed at a step's end: L <= 64) is ONE match of distance 1 when L >= 3 -- the standard length code and extra bits, then
 *     distance code 0, five zero bits -- and L literals when L is 1 or 2.  Every other byte is a literal, standard fixed codes;
 *   - what the bytes depend on: the raster alone -- identical for every MARAY_PNG_BAND_ROWS, stream and call;
 *   - Adler-32: over the filtered bytes as above, by the same per-segment shares; a band's byte count is rows (rb + 1).
 * The modes: MARAY_PNG_COLOR_RGB is exactly the plain entry point.  MARAY_PNG_COLOR_INDEXED writes the indexed file; a raster
 * of more than 256 colours is MARAY_E_LIMIT ("more than 256 colours"), no file is produced and the encoder stays usable.
 * MARAY_PNG_COLOR_AUTO writes the indexed file where it exists and otherwise exactly the RGB file.  This family is fixed codes
 * and filter 0 only.  An unknown mode or a reserved word that is not 0 is MARAY_E_ARG, reported before a device is looked for.
 * How it runs: maray_png_colors (a capped grid; every block collects its pixels' colours in a set in LDS and stores them to
 * a slab of its own) and maray_png_colors_merge (one block: the slabs' union, and the palette of earlier bands, ranked) over
 * the whole raster; one copy of 1,028 bytes (the count and the palette) and a wait; the decision; then per band
 * maray_png_index (RGB8 rows -> packed index rows in an encoder-owned buffer), maray_png_compress_idx (the tokeniser above,
 * one wavefront per segment), maray_png_scan, maray_png_gather and the two copies of the truecolour path.
 * maray_hip_render_png_color renders an image that fits one band ONCE and encodes it from the band buffer; a taller image is
 * rendered TWICE per band, first to collect the colours, then to encode (rendering is deterministic for given values, the
 * shutter form included); with MARAY_PNG_COLOR_AUTO and more than 256 colours the second pass is the truecolour path.
 * maray_gen, the CLI and the animation writers do not take the mode. */
enum { MARAY_PNG_COLOR_RGB = 0, MARAY_PNG_COLOR_INDEXED = 1, MARAY_PNG_COLOR_AUTO = 2 };
typedef struct { uint32_t color, reserved[7]; } maray_png_color_opts;     /* 32 bytes; null = all zeros */
int maray_hip_png_encode_device_color(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_color_opts *opts, void *stream, uint8_t **png_out, size_t *n_out);
int maray_hip_render_png_color(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, const maray_png_color_opts *opts, uint8_t **png_out, size_t *n_out);
/* all the kernels of one band, the collection included (the palette is fetched once, before the timed loop); with
 * MARAY_PNG_COLOR_AUTO on more than 256 colours: the collection's kernels plus the truecolour band's */
int maray_hip_time_png_encode_color(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_color_opts *opts, int reps, float *ms_avg, uint64_t *stream_bytes);
/* The sorted palette alone: *n_colors = the count, or 257 for "more than 256" (the palette's contents are then unspecified);
 * up to 256 entries of R, G, B.  maray_hip_png_bytes_to_host counts the palette's 1,028 bytes too. */
int maray_hip_png_palette(int device, const void *d_rgb8, uint32_t w, uint32_t h, void *stream, uint32_t *n_colors, uint8_t palette[768]);

/* ---- animation (one APNG, encoded on the device frame by frame) ----------------------------------------------------
 * An animation is written as ONE file: an APNG, i.e. a PNG whose IDAT image is frame 0 (any PNG reader shows it) followed
 * by the later frames, each a complete zlib stream -- the device PNG encoder's, above -- of a SUB-RECTANGLE of the canvas.
 * The rectangle of frame i > 0 is the bounding box of the pixels in which it differs from frame i - 1, found on the device
 * (maray_frame_delta): only that rectangle is compressed and copied to the host, plus the box's 16 bytes.
 *   - container: signature; IHDR (w, h, 8, 2, 0, 0, 0); acTL (num_frames u32, num_plays u32; 0 plays = for ever); fcTL
 *     (sequence 0, w x h at 0, 0) and frame 0's stream in IDAT chunks of at most 2^30 bytes; for every later frame fcTL and
 *     fdAT chunks of a 4-byte sequence number and at most 2^30 - 4 bytes of the stream; IEND.  fcTL is 26 bytes: sequence,
 *     width, height, x_offset, y_offset (u32 each), delay_num, delay_den (u16), dispose_op 0 (NONE), blend_op 0 (SOURCE).
 *     Sequence numbers are shared by fcTL and fdAT: 0, 1, 2, ... without a gap.  All words big-endian, CRC-32 by zlib's crc32;
 *   - a frame equal to the one before it is written as the 1 x 1 rectangle at (0, 0): APNG has no empty frame, and a SOURCE
 *     blend of an unchanged pixel changes nothing;
 *   - a frame's stream is closed like a still's: 78 01, its segments, 01 00 00 FF FF, the Adler-32 of its filtered bytes
 *     (rows of one filter byte and 3 bw bytes, bw the rectangle's width);
 *   - the file is a function of the frames' rasters, delay_num, delay_den and n_plays alone: the same bytes for every
 *     MARAY_PNG_BAND_ROWS and every stream;
 *   - every frame shows for delay_num / delay_den seconds (delay_den = 0 means 100, by the APNG specification).
 * maray_frame_delta's contract: two packed RGB8 rasters of w x h pixels in device memory, row pitch exactly 3 w, any byte
 * alignment, independently; box = x0, y0, x1, y1, the half-open bounding box of all pixels in which any of the three bytes
 * differs, and 0, 0, 0, 0 when no byte differs.  Exact.  Nothing is written but the box (and the call's partial boxes).
 * How it runs: the writer holds two whole-frame rasters on the device and swaps them between frames; per frame the render
 * in the encoder's band steps, maray_frame_delta + maray_frame_delta_box, one copy of 16 bytes, a 2-D device-to-device copy
 * of the box's rows into the encoder's band buffer (left out where the box is as wide as the canvas) and the encoder's
 * kernels and copies per band.  One device per animation.
 * Errors: n_images (n_frames) = 0, delay_num or delay_den above 65535, a null pointer, w = 0 or h = 0: MARAY_E_ARG; the
 * device PNG encoder's size limits per frame, and a frame of more than 2^30 bytes (3 w h): MARAY_E_LIMIT; nothing is
 * launched in those cases. */
/* The kernel alone on the caller's rasters: enqueued on `stream` (NULL = the null stream) and waited for. */
int maray_hip_frame_delta(int device, const void *d_prev, const void *d_cur, uint32_t w, uint32_t h, void *stream, uint32_t box[4]);
/* n_frames packed frames, 3 w h bytes apart, already in device memory at any alignment -> a complete APNG in malloc'ed host
 * memory (maray_free): the animation twin of maray_hip_png_encode_device. */
int maray_hip_apng_encode_device(int device, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, uint32_t delay_num,
                                 uint32_t delay_den, uint32_t n_plays, void *stream, uint8_t **out, size_t *n_out);
/* n_images images of a context (any back-end, samples, filter, transfer) as an APNG.  `values` is an (n_images * n_sub) x P
 * matrix, P = the program's parameter count: image i is the shutter render ("shutter" above) over its n_sub rows; n_sub = 1
 * is the plain render with that row, and n_sub is 1, 2, 4, ..., 64.  Every row is checked against the declared ranges
 * before the first launch (MARAY_E_ARG, nothing rendered); the context's own values are unchanged afterwards.  A program
 * without parameters takes values = NULL and renders n_images equal images. */
int maray_hip_render_apng(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub,
                          uint32_t delay_num, uint32_t delay_den, uint32_t n_plays, uint8_t **out, size_t *n_out);
/* Measurements: average ms of maray_frame_delta + maray_frame_delta_box over two w x h rasters of the call's own that
 * differ in their first and last byte (maray_hip_time_filter's fill).  maray_hip_time_frame_delta_copy also times, in the
 * same call, a device-to-device hipMemcpyAsync of one raster's bytes -- the same 2 x 3 w h bytes moved. */
int maray_hip_time_frame_delta(int device, uint32_t w, uint32_t h, int reps, float *ms_avg);
int maray_hip_time_frame_delta_copy(int device, uint32_t w, uint32_t h, int reps, float *ms_avg, float *copy_ms_avg);
/* gen for an animation: image i is the scene with its parameters set to row i of `values` (n_images x the scene's declared
 * parameter count), written to `path` as one APNG.  With opts->shutter = n > 1 each image's sub-frames are the scene's
 * maray_scene_shutter_values around that row.  The tape and the context come from what maray_gen_to_image keeps, exactly as
 * it finds them: a second animation of a scene pays no lowering.  One device: opts->n_devices > 1 is MARAY_E_ARG;
 * opts->encoder is ignored (an animation is always encoded on the device) but for the flag MARAY_ENCODER_DYNAMIC: dynamic
 * codes for every frame; there are no progress reports.  The scene's
 * current parameter values are as they were when the call returns, however it ends. */
int maray_gen_animation(const maray_scene *s, const maray_texture *tex, uint32_t n_tex, const maray_gen_opts *opts, const double *values,
                        uint32_t n_images, uint32_t delay_num, uint32_t delay_den, uint32_t n_plays, const char *path);

/* ---- raw video (an animation as YUV4MPEG2: RGB -> Y'CbCr on the device) ----------------------------------------------
 * What a video encoder reads (ffmpeg, x264, SVT-AV1, aomenc): uncompressed planar Y'CbCr behind a one-line text header.
 * The conversion runs on the device (maray_rgb_to_ycc), so that 1.5 bytes a pixel cross to the host at 4:2:0, not 3, and
 * no compressor stands in the way: this path creates no PNG encoder.
 * Conversion.  Input: a packed RGB8 raster, w x h, row pitch exactly 3 w, at any byte alignment.  Output: three packed
 * planes one after the other, no padding, at any alignment: Y' (w h bytes), Cb, Cr -- exactly the payload of one Y4M FRAME.
 *   - sampling: MARAY_YCC_420 (default): Cb and Cr are cw x ch, cw = (w + 1) / 2, ch = (h + 1) / 2 (integer division);
 *     MARAY_YCC_444: Cb and Cr are w x h;
 *   - matrix: MARAY_YCC_BT601 (default) or MARAY_YCC_BT709, both limited range.  Coefficient rows (y; cb; cr):
 *       BT.601: (66, 129, 25; -38, -74, 112; 112, -94, -18)       BT.709: (47, 157, 16; -26, -86, 112; 112, -102, -10)
 *     (each luma row sums to 220, each chroma row to 0);
 *   - luma: Y' = ((y . (R, G, B) + 128) >> 8) + 16 for every pixel;
 *   - chroma at 4:4:4: C = ((c . (R, G, B) + 128) >> 8) + 128;
 *   - chroma at 4:2:0: Rs, Gs, Bs are the sums over the four pixels (min(2i + a, w - 1), min(2j + b, h - 1)), a, b in {0, 1}
 *     -- indices are clamped to the image, never to a launch -- and C = ((c . (Rs, Gs, Bs) + 512) >> 10) + 128: chroma is
 *     sited at the centre of the 2 x 2 block (C420jpeg);
 *   - >> is an arithmetic shift (floor) of a signed 32-bit value.  Everything is an integer: the planes are the same for
 *     every launch shape, stream and alignment.  Over all 2^24 colours Y' is in [16, 235] and Cb, Cr in [16, 240] (at 4:2:0
 *     as well), greys give Cb = Cr = 128 exactly: there is no clamp.  The largest distance from the real-valued definition
 *     is 0.76 of a code value in Y' and 0.99 in Cb/Cr (BT.601), 0.88 and 1.17 (BT.709).
 * Container.  One header line, `YUV4MPEG2 W<w> H<h> F<fn>:<fd> Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n` (C444 at 4:4:4);
 * then per frame `FRAME\n` and the planes.  fn:fd = delay_den:delay_num, delay_den = 0 meaning 100 as for the APNG; the
 * fraction is not reduced.  The file is a function of the frames' rasters, the two delays, the sampling and the matrix alone.
 * Y4M has no tag for the matrix: the caller tells the consumer which one it chose.
 * How it runs: two plane buffers on the device and two in pinned host memory; per frame the render (through the context's
 * device entry points; the shutter's for n_sub > 1), the conversion on the same stream, an event, and the planes' copy on a
 * copy stream; frame k - 1 is written by the calling thread while frame k renders.  One device per animation.
 * Errors, before a device is looked for: a null pointer, w = 0 or h = 0, n_frames = 0, delay_num = 0, a delay above 65535, an
 * unknown sampling, matrix or container, a reserved word that is not 0, n_devices > 1: MARAY_E_ARG; a side above
 * MARAY_DOMAIN_MAX, 3 w h above 2^30: MARAY_E_LIMIT.  Nothing is launched in those cases. */
#define MARAY_YCC_420 0u
#define MARAY_YCC_444 1u
#define MARAY_YCC_BT601 0u
#define MARAY_YCC_BT709 1u
#define MARAY_CONTAINER_APNG 0u
#define MARAY_CONTAINER_Y4M 1u
typedef struct maray_ycc_opts { uint32_t sampling, matrix, reserved[6]; } maray_ycc_opts;        /* a null pointer: all zeros */
typedef struct maray_anim_opts { uint32_t container, sampling, matrix, reserved[5]; } maray_anim_opts;
/* Bytes of one frame's three planes: w h + 2 cw ch.  Needs no device. */
int maray_ycc_frame_bytes(uint32_t w, uint32_t h, uint32_t sampling, size_t *out);
/* The kernel alone: the caller's raster to the caller's planes (maray_ycc_frame_bytes of them), enqueued on `stream` (NULL =
 * the null stream) of `device`; it does not synchronise. */
int maray_hip_rgb_to_ycc(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_ycc_opts *opts, void *d_planes, void *stream);
/* n_frames packed frames, 3 w h bytes apart, already in device memory at any alignment -> a complete Y4M file in malloc'ed
 * host memory (maray_free): the twin of maray_hip_apng_encode_device. */
int maray_hip_y4m_encode_device(int device, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, uint32_t delay_num,
                                uint32_t delay_den, const maray_ycc_opts *opts, void *stream, uint8_t **out, size_t *n_out);
/* n_images images of a context as a Y4M file; `values` and n_sub exactly as maray_hip_render_apng takes them. */
int maray_hip_render_y4m(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub,
                         uint32_t delay_num, uint32_t delay_den, const maray_ycc_opts *opts, uint8_t **out, size_t *n_out);
/* Measurement: average ms of maray_rgb_to_ycc over a w x h raster of the call's own (maray_hip_time_filter's fill) and, in
 * the same call, of a device-to-device hipMemcpyAsync that moves as many bytes: 4.5 w h at 4:2:0 and 6 w h at 4:4:4 (a copy
 * of half as many).  copy_ms_avg may be null. */
int maray_hip_time_rgb_to_ycc(int device, uint32_t w, uint32_t h, const maray_ycc_opts *opts, int reps, float *ms_avg, float *copy_ms_avg);
/* maray_gen_animation with a container (maray_gen_opts has no spare word).  a = NULL or a->container = MARAY_CONTAINER_APNG:
 * maray_gen_animation, byte for byte.  MARAY_CONTAINER_Y4M: the images as one Y4M file, streamed to `path` frame by frame --
 * host memory is two frames, not the whole file; n_plays and the flag MARAY_ENCODER_DYNAMIC are ignored; an error leaves no
 * file. */
int maray_gen_animation_ex(const maray_scene *s, const maray_texture *tex, uint32_t n_tex, const maray_gen_opts *opts, const double *values,
                           uint32_t n_images, uint32_t delay_num, uint32_t delay_den, uint32_t n_plays, const maray_anim_opts *a, const char *path);

/* PNG I/O used by gen and the CLI (`img.save`, `image::open(..).to_rgb8()`). */
int maray_png_write(const char *path, const uint8_t *rgb8, uint32_t w, uint32_t h);
int maray_png_read(const char *path, uint8_t **rgb8_out, uint32_t *w, uint32_t *h);   /* free with maray_free */
/* `image::open(file).unwrap().to_rgb8()` (examples/maray.rs:58-65): a texture in any format this library reads -- told from
 * the file's first bytes like the `image` crate does: PNG, BMP, PNM (P1 - P6), TGA, QOI, farbfeld, GIF (the first frame),
 * TIFF (grey / RGB strips) -- as RGB8 (alpha dropped, grey replicated, 16-bit samples rounded).  JPEG / WebP:
 * MARAY_E_DECODE naming the format. */
int maray_image_read(const char *path, uint8_t **rgb8_out, uint32_t *w, uint32_t *h);   /* free with maray_free */
void maray_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
