"""ctypes binding of libmaray_hip.so — host-side mirror of the reference's render
surface (`open`, `save`, `gen`, `gen_to_image`, `RenderMethod`; src/lib.rs:1155-1235).

Plumbing only: no arithmetic happens here.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
OP_COUNT = 20
BACKEND_TAPE, BACKEND_TAPE_SMEM, BACKEND_JIT, BACKEND_AUTO = 0, 1, 2, 3
REPORT_NONE, REPORT_ROW, REPORT_DURATION_MS = 0, 1, 2
FILTER_BOX, FILTER_TENT, FILTER_CATROM = 0, 1, 3        # (2 is unassigned: refused)
ENCODER_HOST, ENCODER_DEVICE = 0, 1
ENCODER_DYNAMIC = 0x100                 # a flag on ENCODER_DEVICE: dynamic-Huffman codes (MARAY_ENCODER_DYNAMIC)
CODES_FIXED, CODES_DYNAMIC = 0, 1       # MARAY_PNG_CODES_*
# MARAY_PNG_FILTER_*: the device PNG encoder's row filter (png_filter=; `filter` is the reconstruction filter everywhere)
PNG_FILTER_NONE, PNG_FILTER_ADAPTIVE, PNG_FILTER_SUB, PNG_FILTER_UP, PNG_FILTER_AVERAGE, PNG_FILTER_PAETH = range(6)
# MARAY_PNG_COLOR_*: the device PNG encoder's colour mode (png_color=): truecolour, indexed, or indexed where at most 256 colours
PNG_COLOR_RGB, PNG_COLOR_INDEXED, PNG_COLOR_AUTO = range(3)
TRANSFER_NONE, TRANSFER_SRGB = 0, 1
YCC_420, YCC_444 = 0, 1                 # MARAY_YCC_*: the chroma sampling of the raw-video planes
YCC_BT601, YCC_BT709 = 0, 1             # ... and their matrix (both limited range)
CONTAINER_APNG, CONTAINER_Y4M = 0, 1    # MARAY_CONTAINER_*: what gen_animation writes


class PngOpts(C.Structure):
    """maray_png_opts"""
    _fields_ = [('codes', C.c_uint32), ('filter', C.c_uint32), ('reserved', C.c_uint32 * 6)]


class PngColorOpts(C.Structure):
    """maray_png_color_opts"""
    _fields_ = [('color', C.c_uint32), ('reserved', C.c_uint32 * 7)]


class YccOpts(C.Structure):
    """maray_ycc_opts"""
    _fields_ = [('sampling', C.c_uint32), ('matrix', C.c_uint32), ('reserved', C.c_uint32 * 6)]


class AnimOpts(C.Structure):
    """maray_anim_opts"""
    _fields_ = [('container', C.c_uint32), ('sampling', C.c_uint32), ('matrix', C.c_uint32), ('reserved', C.c_uint32 * 5)]


def _ycc_opts(sampling, matrix):
    o = YccOpts()
    o.sampling, o.matrix = sampling, matrix
    return o


def _png_opts(codes, png_filter):
    o = PngOpts()
    o.codes, o.filter = codes, png_filter
    return o


def _png_color_opts(png_color, codes, png_filter, who):
    """The options of the `_color` family, which is fixed codes and filter 0 only."""
    if codes != CODES_FIXED or png_filter != PNG_FILTER_NONE:
        raise MarayError(-1, '%s: a png_color mode takes neither codes nor png_filter' % who)
    o = PngColorOpts()
    o.color = png_color
    return o


class MarayError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('maray error %d: %s' % (code, msg))
        self.code = code


class Refine(C.Structure):
    """maray_refine (include/maray_tape.h): a program's REFINE section, beside its Program (whose layout is unchanged)."""
    _fields_ = [('n_consts', C.c_uint32), ('consts', C.POINTER(C.c_double)), ('n_ops', C.c_uint32), ('ops', C.POINTER(C.c_uint64)),
                ('n_slots', C.c_uint32), ('n_outs', C.c_uint32)]


class Program(C.Structure):
    _fields_ = [('version', C.c_uint32), ('n_consts', C.c_uint32), ('consts', C.POINTER(C.c_double)),
                ('n_row_ops', C.c_uint32), ('row_ops', C.POINTER(C.c_uint64)), ('n_row_slots', C.c_uint32),
                ('n_yvals', C.c_uint32), ('n_pix_ops', C.c_uint32), ('pix_ops', C.POINTER(C.c_uint64)),
                ('n_pix_slots', C.c_uint32), ('n_app', C.c_uint32),
                # version 3 only (include/maray_tape.h): a version-2 struct ends at n_app
                ('n_params', C.c_uint32), ('param_ranges', C.POINTER(C.c_double))]


class TapeInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ('n_consts', 'n_row_ops', 'n_row_slots', 'n_yvals', 'n_pix_ops', 'n_pix_slots', 'n_app', 'alg_ops',
                 'alg_ops_xy', 'alg_ops_x', 'alg_ops_y', 'alg_ops_uniform', 'folded_ops', 'dag_nodes',
                 'acc_operands', 'skip_ops', 'bool_ops', 'sin_ops', 'sin_bounded', 'private_regions', 'rebalanced_chains')] + \
               [('op_histogram', C.c_uint32 * OP_COUNT), ('row_params_words', C.c_uint32 * 2)]


class Texture(C.Structure):
    _fields_ = [('rgb', C.c_void_p), ('w', C.c_uint32), ('h', C.c_uint32)]


class LowerOpts(C.Structure):
    _fields_ = [('hoist_rows', C.c_uint32), ('plain_cse', C.c_uint32), ('no_fuse', C.c_uint32), ('no_skips', C.c_uint32), ('no_row_guards', C.c_uint32),
                ('no_private_regions', C.c_uint32), ('no_rebalance', C.c_uint32), ('no_y_spans', C.c_uint32)]


class CtxOpts(C.Structure):
    _fields_ = [('backend', C.c_uint32), ('hint_mpixels', C.c_uint32), ('samples', C.c_uint32), ('filter', C.c_uint32), ('transfer', C.c_uint32),
                ('reserved', C.c_uint32 * 3)]


class GenOpts(C.Structure):
    _fields_ = [('backend', C.c_uint32), ('n_devices', C.c_uint32), ('tile_rows', C.c_uint32), ('samples', C.c_uint32),
                ('shutter', C.c_uint32), ('filter', C.c_uint32), ('encoder', C.c_uint32), ('transfer', C.c_uint32)]


class Report(C.Structure):
    _fields_ = [('kind', C.c_uint32), ('value', C.c_uint32)]


REPORT_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_double)
TILE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32)

_lib = None


def lib_path():
    return os.path.join(_HERE, 'libmaray_hip.so')


def lib():
    """Load libmaray_hip.so; fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise MarayError(-8, 'libmaray_hip.so is not built (run `make -C maray_amd/csrc` or __graft_entry__.build())')
    L = C.CDLL(p)
    vp, u32, u64p = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)
    sig = {
        'maray_last_error': (C.c_char_p, []),
        'maray_version': (C.c_char_p, []),
        'maray_scene_open': (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        'maray_scene_from_bytes': (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(vp)]),
        'maray_scene_free': (None, [vp]),
        'maray_scene_size': (C.c_int, [vp, C.POINTER(u32), C.POINTER(u32)]),
        'maray_scene_set_size': (C.c_int, [vp, u32, u32]),
        'maray_scene_is_legacy': (C.c_int, [vp, C.POINTER(C.c_int)]),
        'maray_scene_node_count': (C.c_int, [vp, C.c_int, u64p]),
        'maray_scene_encode': (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        'maray_scene_save': (C.c_int, [vp, C.c_char_p]),
        'maray_scene_fix_color': (C.c_int, [vp]),
        'maray_scene_rescale': (C.c_int, [vp, u32, u32]),
        'maray_scene_supersample': (C.c_int, [vp, u32]),
        'maray_scene_simplify': (C.c_int, [vp]),
        'maray_scene_simplify_ex': (C.c_int, [vp, C.c_uint32]),
        'maray_scene_compress': (C.c_int, [vp, C.POINTER(u32)]),
        'maray_scene_display_len': (C.c_int, [vp, C.c_int, u64p]),
        'maray_var_id': (C.c_uint64, [C.c_char_p]),
        'maray_scene_declare_param': (C.c_int, [vp, C.c_uint64, C.c_double, C.c_double, C.POINTER(u32)]),
        'maray_scene_param_count': (C.c_int, [vp, C.POINTER(u32)]),
        'maray_scene_param_info': (C.c_int, [vp, u32, u64p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        'maray_scene_set_param': (C.c_int, [vp, u32, C.c_double]),
        'maray_scene_set_param_span': (C.c_int, [vp, u32, C.c_double]),
        'maray_scene_param_span': (C.c_int, [vp, u32, C.POINTER(C.c_double)]),
        'maray_scene_shutter_values': (C.c_int, [vp, u32, vp]),
        'maray_hip_render_rows_shutter': (C.c_int, [vp, u32, u32, u32, u32, vp, u32, vp]),
        'maray_hip_render_rows_shutter_device': (C.c_int, [vp, u32, u32, u32, u32, vp, u32, vp, vp]),
        'maray_hip_render_tiles_shutter': (C.c_int, [vp, u32, u32, C.POINTER(u32), u32, vp, u32, vp, TILE_FN, vp]),
        'maray_hip_time_shutter_reduce': (C.c_int, [C.c_int, C.c_size_t, u32, C.c_int, C.POINTER(C.c_float)]),
        'maray_hip_time_filter': (C.c_int, [C.c_int, u32, u32, u32, C.c_int, C.POINTER(C.c_float)]),
        'maray_hip_time_filter_ex': (C.c_int, [C.c_int, u32, u32, u32, u32, u32, C.c_int, C.POINTER(C.c_float)]),
        'maray_hip_time_shutter_reduce_ex': (C.c_int, [C.c_int, C.c_size_t, u32, u32, C.c_int, C.POINTER(C.c_float)]),
        'maray_transfer_table': (C.c_int, [u32, vp, vp]),
        'maray_tape_param_count': (C.c_int, [vp, C.POINTER(u32)]),
        'maray_tape_param_range': (C.c_int, [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        'maray_hip_ctx_set_params': (C.c_int, [vp, C.POINTER(C.c_double), u32]),
        'maray_hip_ctx_param_count': (C.c_int, [vp, C.POINTER(u32)]),
        'maray_lower': (C.c_int, [vp, C.POINTER(LowerOpts), C.POINTER(vp)]),
        'maray_tape_free': (None, [vp]),
        'maray_tape_program': (C.c_int, [vp, C.POINTER(Program)]),
        'maray_tape_get_info': (C.c_int, [vp, C.POINTER(TapeInfo)]),
        'maray_hip_device_count': (C.c_int, [C.POINTER(C.c_int)]),
        'maray_hip_ctx_create': (C.c_int, [C.c_int, C.POINTER(Program), C.POINTER(Texture), u32, C.POINTER(CtxOpts),
                                           C.POINTER(vp)]),
        'maray_hip_ctx_create_refined': (C.c_int, [C.c_int, C.POINTER(Program), C.POINTER(Refine), C.POINTER(Texture), u32, C.POINTER(CtxOpts),
                                                   C.POINTER(vp)]),
        'maray_tape_refine': (C.c_int, [vp, C.POINTER(Refine)]),
        'maray_jit_source_refine': (C.c_int, [C.POINTER(Program), C.POINTER(Refine), C.POINTER(vp)]),
        'maray_jit_build_refine': (C.c_int, [C.POINTER(Program), C.POINTER(Refine), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_jit_guard_layout': (C.c_int, [C.POINTER(Program), vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        'maray_hip_refine_count': (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        'maray_hip_census_count': (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        'maray_jit_census_eligible': (C.c_int, [C.POINTER(Program), vp, u32, C.POINTER(u32)]),
        'maray_jit_source_census': (C.c_int, [C.POINTER(Program), C.POINTER(vp)]),
        'maray_hip_debug_guard_words': (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(u32)]),
        'maray_hip_debug_census_words': (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(u32)]),
        'maray_hip_cover_count': (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        'maray_jit_cover_bits': (C.c_int, [C.POINTER(Program), vp, u32, C.POINTER(u32)]),
        'maray_jit_source_cover': (C.c_int, [C.POINTER(Program), C.POINTER(vp)]),
        'maray_hip_debug_cover_words': (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(u32)]),
        'maray_hip_rowscan_count': (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        'maray_jit_rowwords_flag': (C.c_int, [C.POINTER(Program), C.POINTER(C.c_int32)]),
        'maray_jit_source_rowwords': (C.c_int, [C.POINTER(Program), C.POINTER(vp)]),
        'maray_hip_prepass_count': (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        'maray_hip_deferred_count': (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        'maray_jit_source_prepass': (C.c_int, [C.POINTER(Program), C.POINTER(vp)]),
        'maray_hip_debug_row_words': (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(u32), C.POINTER(C.c_int)]),
        'maray_hip_debug_row_sets': (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(u32), u64p, u64p, u64p]),
        'maray_hip_ctx_free': (None, [vp]),
        'maray_hip_render_rows': (C.c_int, [vp, u32, u32, u32, u32, vp, vp]),
        'maray_hip_render_tiles': (C.c_int, [vp, u32, u32, C.POINTER(u32), u32, vp, TILE_FN, vp]),
        'maray_host_alloc': (C.c_int, [C.c_size_t, C.POINTER(vp)]),
        'maray_host_free': (None, [vp]),
        'maray_host_register': (C.c_int, [vp, C.c_size_t]),
        'maray_host_unregister': (C.c_int, [vp]),
        'maray_hip_render_rows_device': (C.c_int, [vp, u32, u32, u32, u32, vp, vp, vp]),
        'maray_hip_render_blocks_device': (C.c_int, [vp, u32, u32, u32, u32, u32, u32, vp, vp, vp]),
        'maray_hip_time_rows': (C.c_int, [vp, u32, u32, u32, u32, vp, vp, C.c_int, C.POINTER(C.c_float)]),
        'maray_hip_time_blocks': (C.c_int, [vp, u32, u32, u32, u32, u32, u32, vp, vp, C.c_int, C.POINTER(C.c_float)]),
        'maray_hip_kernel_name': (C.c_char_p, [vp]),
        'maray_hip_launch_counts': (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        'maray_jit_code_key': (C.c_int, [C.POINTER(Program), C.c_char_p]),
        'maray_jit_code_cached': (C.c_int, [C.POINTER(Program), C.POINTER(C.c_int)]),
        'maray_gen_to_image': (C.c_int, [vp, C.POINTER(Texture), u32, C.POINTER(GenOpts), Report, REPORT_FN, vp, vp,
                                         u32, u32]),
        'maray_gen': (C.c_int, [vp, C.POINTER(Texture), u32, C.POINTER(GenOpts), Report, C.c_char_p]),
        'maray_gen_cache_clear': (None, []),
        'maray_gen_cache_info': (C.c_int, [C.c_char_p, C.c_size_t]),
        'maray_hip_png_encode_device': (C.c_int, [C.c_int, vp, u32, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_render_png': (C.c_int, [vp, u32, u32, vp, u32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_time_png_encode': (C.c_int, [C.c_int, vp, u32, u32, C.c_int, C.POINTER(C.c_float), u64p]),
        'maray_hip_png_encode_device_ex': (C.c_int, [C.c_int, vp, u32, u32, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_render_png_ex': (C.c_int, [vp, u32, u32, vp, u32, u32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_time_png_encode_ex': (C.c_int, [C.c_int, vp, u32, u32, u32, C.c_int, C.POINTER(C.c_float), u64p]),
        'maray_hip_png_encode_device_opts': (C.c_int, [C.c_int, vp, u32, u32, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_render_png_opts': (C.c_int, [vp, u32, u32, vp, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_time_png_encode_opts': (C.c_int, [C.c_int, vp, u32, u32, vp, C.c_int, C.POINTER(C.c_float), u64p]),
        'maray_hip_png_encode_device_color': (C.c_int, [C.c_int, vp, u32, u32, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_render_png_color': (C.c_int, [vp, u32, u32, vp, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_time_png_encode_color': (C.c_int, [C.c_int, vp, u32, u32, vp, C.c_int, C.POINTER(C.c_float), u64p]),
        'maray_hip_png_palette': (C.c_int, [C.c_int, vp, u32, u32, vp, C.POINTER(u32), vp]),
        'maray_png_dynamic_codes': (C.c_int, [vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        'maray_hip_png_bytes_to_host': (C.c_uint64, []),
        'maray_hip_frame_delta': (C.c_int, [C.c_int, vp, vp, u32, u32, vp, C.POINTER(u32)]),
        'maray_hip_apng_encode_device': (C.c_int, [C.c_int, vp, u32, u32, u32, u32, u32, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_render_apng': (C.c_int, [vp, u32, u32, vp, u32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_time_frame_delta': (C.c_int, [C.c_int, u32, u32, C.c_int, C.POINTER(C.c_float)]),
        'maray_hip_time_frame_delta_copy': (C.c_int, [C.c_int, u32, u32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        'maray_gen_animation': (C.c_int, [vp, C.POINTER(Texture), u32, C.POINTER(GenOpts), vp, u32, u32, u32, u32, C.c_char_p]),
        'maray_ycc_frame_bytes': (C.c_int, [u32, u32, u32, C.POINTER(C.c_size_t)]),
        'maray_hip_rgb_to_ycc': (C.c_int, [C.c_int, vp, u32, u32, C.POINTER(YccOpts), vp, vp]),
        'maray_hip_y4m_encode_device': (C.c_int, [C.c_int, vp, u32, u32, u32, u32, u32, C.POINTER(YccOpts), vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_render_y4m': (C.c_int, [vp, u32, u32, vp, u32, u32, u32, u32, C.POINTER(YccOpts), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        'maray_hip_time_rgb_to_ycc': (C.c_int, [C.c_int, u32, u32, C.POINTER(YccOpts), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        'maray_gen_animation_ex': (C.c_int, [vp, C.POINTER(Texture), u32, C.POINTER(GenOpts), vp, u32, u32, u32, u32, C.POINTER(AnimOpts), C.c_char_p]),
        'maray_png_write': (C.c_int, [C.c_char_p, vp, u32, u32]),
        'maray_png_read': (C.c_int, [C.c_char_p, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]),
        'maray_image_read': (C.c_int, [C.c_char_p, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]),
        'maray_free': (None, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise MarayError(rc, lib().maray_last_error().decode(errors='replace'))


def version():
    return lib().maray_version().decode()


def device_count():
    n = C.c_int(0)
    _check(lib().maray_hip_device_count(C.byref(n)))
    return n.value


def var_id(name):
    """The id `var(name)` makes (src/lib.rs:845-850)."""
    return lib().maray_var_id(name.encode())


def _param_id(name_or_id):
    return var_id(name_or_id) if isinstance(name_or_id, str) else int(name_or_id)


def _textures(textures):
    if not textures:
        return None, 0, []
    keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
    arr = (Texture * len(keep))()
    for i, t in enumerate(keep):
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError('textures must be HxWx3 uint8')
        arr[i].rgb = t.ctypes.data
        arr[i].w = t.shape[1]
        arr[i].h = t.shape[0]
    return arr, len(keep), keep


class Scene:
    """`([u32;2], [Expr;3])` as read by `maray::open` (src/lib.rs:1227-1235)."""

    def __init__(self, data=None, path=None):
        h = C.c_void_p()
        if path is not None:
            _check(lib().maray_scene_open(os.fsencode(path), C.byref(h)))
        else:
            _check(lib().maray_scene_from_bytes(data, len(data), C.byref(h)))
        self._h = h

    @classmethod
    def open(cls, path):
        return cls(path=path)

    def __del__(self):
        if getattr(self, '_h', None):
            lib().maray_scene_free(self._h)
            self._h = None

    @property
    def size(self):
        w, h = C.c_uint32(), C.c_uint32()
        _check(lib().maray_scene_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def set_size(self, w, h):
        _check(lib().maray_scene_set_size(self._h, w, h))

    @property
    def legacy(self):
        v = C.c_int()
        _check(lib().maray_scene_is_legacy(self._h, C.byref(v)))
        return bool(v.value)

    def node_count(self, c):
        n = C.c_uint64()
        _check(lib().maray_scene_node_count(self._h, c, C.byref(n)))
        return n.value

    def encode(self):
        n = C.c_size_t()
        _check(lib().maray_scene_encode(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().maray_scene_encode(self._h, buf, n.value, C.byref(n)))
        return buf.raw

    def save(self, path):
        _check(lib().maray_scene_save(self._h, os.fsencode(path)))

    def fix_color(self):
        _check(lib().maray_scene_fix_color(self._h))

    def simplify(self, merge_divisors=False):
        """Expr::simplify on each channel (authoring-time rewrite rules of the reference).  merge_divisors: the one rewrite
        the reference lacks, without which its rules do not terminate on examples/chess.rs (maray_hip.h)."""
        if merge_divisors:
            _check(lib().maray_scene_simplify_ex(self._h, 1))
        else:
            _check(lib().maray_scene_simplify(self._h))

    def compress(self):
        """Expr::compress on each channel (authoring-time: names repeated sub-expressions); returns the variables introduced."""
        n = (C.c_uint32 * 3)()
        _check(lib().maray_scene_compress(self._h, n))
        return list(n)

    def display_len(self, c):
        """Characters of the reference's printed form of channel c."""
        n = C.c_uint64()
        _check(lib().maray_scene_display_len(self._h, c, C.byref(n)))
        return n.value

    def rescale(self, sx, sy):
        _check(lib().maray_scene_rescale(self._h, sx, sy))

    def supersample(self, k):
        """The scene on a k x k finer grid, centred on the plain one (k = 1, 2, 4, 8; 0 and 1 change nothing): what a
        Context(..., samples=k) reduces."""
        _check(lib().maray_scene_supersample(self._h, k))

    # ---- parameters (include/maray_hip.h, "scene parameters") ----
    def declare_param(self, name_or_id, lo=float('-inf'), hi=float('inf')):
        """Declares the free variable `var(name)` (or a raw id) as a run-time parameter with values in [lo, hi]; returns
        its index.  Declaring it again with the same range returns the same index."""
        k = C.c_uint32()
        _check(lib().maray_scene_declare_param(self._h, _param_id(name_or_id), lo, hi, C.byref(k)))
        return k.value

    @property
    def param_count(self):
        n = C.c_uint32()
        _check(lib().maray_scene_param_count(self._h, C.byref(n)))
        return n.value

    def param_info(self, index):
        """(var id, lo, hi, current value) of parameter `index`."""
        i, lo, hi, v = C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
        _check(lib().maray_scene_param_info(self._h, index, C.byref(i), C.byref(lo), C.byref(hi), C.byref(v)))
        return i.value, lo.value, hi.value, v.value

    def param_index(self, name_or_id):
        want = _param_id(name_or_id)
        for k in range(self.param_count):
            if self.param_info(k)[0] == want:
                return k
        raise KeyError(name_or_id)

    def set_param(self, index_or_name, value):
        """The value gen / gen_to_image render parameter `index` (or the parameter declared for a name) with."""
        k = self.param_index(index_or_name) if isinstance(index_or_name, str) else index_or_name
        _check(lib().maray_scene_set_param(self._h, k, value))

    # ---- shutter (include/maray_hip.h, "shutter") ----
    def set_param_span(self, name_or_index, span):
        """The width of the interval of values, centred on the parameter's value, that the frames of a shutter render cover
        (finite, >= 0; 0: every frame has the value itself)."""
        k = self.param_index(name_or_index) if isinstance(name_or_index, str) else name_or_index
        _check(lib().maray_scene_set_param_span(self._h, k, span))

    def param_span(self, index):
        v = C.c_double()
        _check(lib().maray_scene_param_span(self._h, index, C.byref(v)))
        return v.value

    def shutter_values(self, n):
        """The (n, P) float64 matrix of the n frames' parameter values around the scene's current ones."""
        out = np.zeros((n, self.param_count), np.float64)
        _check(lib().maray_scene_shutter_values(self._h, n, out.ctypes.data if out.size else None))
        return out

    def lower(self, hoist_rows=True, plain_cse=False, fuse=True, skips=True, row_guards=True, private_regions=True, rebalance=True,
              y_spans=True):
        return Tape(self, hoist_rows, plain_cse, fuse, skips, row_guards, private_regions, rebalance, y_spans)


class Tape:
    """Lowered program (include/maray_tape.h)."""

    def __init__(self, scene, hoist_rows=True, plain_cse=False, fuse=True, skips=True, row_guards=True, private_regions=True, rebalance=True,
                 y_spans=True):
        o = LowerOpts()
        o.hoist_rows = 1 if hoist_rows else 0
        o.plain_cse = 1 if plain_cse else 0
        o.no_fuse = 0 if fuse else 1
        o.no_skips = 0 if skips else 1
        o.no_row_guards = 0 if row_guards else 1
        o.no_private_regions = 0 if private_regions else 1
        o.no_rebalance = 0 if rebalance else 1
        o.no_y_spans = 0 if y_spans else 1
        h = C.c_void_p()
        _check(lib().maray_lower(scene._h, C.byref(o), C.byref(h)))
        self._h = h
        self.program = Program()
        _check(lib().maray_tape_program(self._h, C.byref(self.program)))
        ti = TapeInfo()
        _check(lib().maray_tape_get_info(self._h, C.byref(ti)))
        self.info = {n: getattr(ti, n) for n, _ in TapeInfo._fields_ if n not in ('op_histogram', 'row_params_words')}
        self.info['op_histogram'] = list(ti.op_histogram)
        self.info['row_params'] = ti.row_params_words[0] | (ti.row_params_words[1] << 32)      # bit p: a ROW op reads PARAM p
        self.refine = Refine()          # the REFINE section (n_ops = 0: none); a Context made from this tape takes it along
        _check(lib().maray_tape_refine(self._h, C.byref(self.refine)))

    def __del__(self):
        if getattr(self, '_h', None):
            lib().maray_tape_free(self._h)
            self._h = None

    @property
    def param_count(self):
        """Parameters of the program: the scene's declared count if some op reads one, else 0."""
        n = C.c_uint32()
        _check(lib().maray_tape_param_count(self._h, C.byref(n)))
        return n.value

    def param_range(self, index):
        lo, hi = C.c_double(), C.c_double()
        _check(lib().maray_tape_param_range(self._h, index, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    @property
    def jit_code_key(self):
        """Cache key of this program's specialised kernels (generated sources + options + hiprtc version)."""
        buf = C.create_string_buffer(33)
        _check(lib().maray_jit_code_key(C.byref(self.program), buf))
        return buf.value.decode()

    @property
    def jit_code_cached(self):
        v = C.c_int()
        _check(lib().maray_jit_code_cached(C.byref(self.program), C.byref(v)))
        return bool(v.value)

    def jit_build_refine(self):
        """The gfx950 code object of maray_jit_refine (bytes; b'' when there is no kernel).  Needs no GPU."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().maray_jit_build_refine(C.byref(self.program), C.byref(self.refine), C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value) if n.value else b''
        finally:
            if p:
                lib().maray_free(p)

    def guard_layout(self):
        """(pos, words, gw, gh) of maray_jit_guard_layout: pos[g] = bit of guard g in a rectangle's words (-1: derived), 64-bit
        words per rectangle, and the rectangle in pixels x rows."""
        n, nw, gw, gh = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().maray_jit_guard_layout(C.byref(self.program), None, 0, C.byref(n), C.byref(nw), C.byref(gw), C.byref(gh)))
        pos = np.zeros(n.value, np.int32)
        _check(lib().maray_jit_guard_layout(C.byref(self.program), pos.ctypes.data, n.value, C.byref(n), C.byref(nw), C.byref(gw), C.byref(gh)))
        return pos, nw.value, gw.value, gh.value

    def census_eligible(self):
        """maray_jit_census_eligible: per guard word of a rectangle (guard_layout), the bits a census may clear, as uint64."""
        n = C.c_uint32()
        _check(lib().maray_jit_census_eligible(C.byref(self.program), None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint64)
        _check(lib().maray_jit_census_eligible(C.byref(self.program), out.ctypes.data, n.value, C.byref(n)))
        return out

    @property
    def jit_source_census(self):
        """Source of maray_jit_census and maray_jit_census_apply; '' when no guard bit is eligible (maray_jit_source_census)."""
        p = C.c_void_p()
        _check(lib().maray_jit_source_census(C.byref(self.program), C.byref(p)))
        try:
            return C.string_at(p).decode()
        finally:
            lib().maray_free(p)

    def cover_plan(self):
        """maray_jit_cover_bits: the boolean ORs of guarded shapes that get a cover bit, a list of dicts {bit, root, leaves}, leaves
        = a list of (last op, guard bit, tainted, eligible).  [] when the program gets none."""
        n = C.c_uint32()
        _check(lib().maray_jit_cover_bits(C.byref(self.program), None, 0, C.byref(n)))
        v = np.zeros(n.value, np.int32)
        _check(lib().maray_jit_cover_bits(C.byref(self.program), v.ctypes.data, n.value, C.byref(n)))
        v, out, at = [int(q) for q in v], [], 1
        for _ in range(v[0]):
            bit, root, nl = v[at:at + 3]
            at += 3
            out.append({'bit': bit, 'root': root, 'leaves': [(v[at + 4 * k], v[at + 4 * k + 1], bool(v[at + 4 * k + 2]), bool(v[at + 4 * k + 3])) for k in range(nl)]})
            at += 4 * nl
        return out

    def cover_bits(self):
        """The cover bits of the program (positions in a rectangle's guard words; none of them is a guard's), one per OR of cover_plan()."""
        return [r['bit'] for r in self.cover_plan()]

    @property
    def jit_source_cover(self):
        """Source of maray_jit_pixels_cov, maray_jit_cover and maray_jit_cover_apply; '' when the program gets no cover bit."""
        p = C.c_void_p()
        _check(lib().maray_jit_source_cover(C.byref(self.program), C.byref(p)))
        try:
            return C.string_at(p).decode()
        finally:
            lib().maray_free(p)

    def rowwords_flag(self):
        """maray_jit_rowwords_flag: the row flag's position in a rectangle's guard words, -1 when the program gets no row words."""
        b = C.c_int32()
        _check(lib().maray_jit_rowwords_flag(C.byref(self.program), C.byref(b)))
        return b.value

    @property
    def jit_source_rowwords(self):
        """Source of maray_jit_pixels_rw and maray_jit_rowscan; '' when the program gets no row words."""
        p = C.c_void_p()
        _check(lib().maray_jit_source_rowwords(C.byref(self.program), C.byref(p)))
        try:
            return C.string_at(p).decode()
        finally:
            lib().maray_free(p)

    @property
    def jit_source_prepass(self):
        """Source of maray_jit_pixels_pp; '' when the program gets no pre-pass."""
        p = C.c_void_p()
        _check(lib().maray_jit_source_prepass(C.byref(self.program), C.byref(p)))
        try:
            return C.string_at(p).decode()
        finally:
            lib().maray_free(p)

    def refine_arrays(self):
        """(consts, ops, n_slots) of the REFINE section as numpy copies; None when the program has none."""
        r = self.refine
        if not r.n_ops:
            return None
        return (np.ctypeslib.as_array(r.consts, shape=(r.n_consts,)).copy(), np.ctypeslib.as_array(r.ops, shape=(r.n_ops,)).copy(), r.n_slots)

    @property
    def jit_source_refine(self):
        """Source of maray_jit_refine; '' when the program gives none (maray_jit_source_refine)."""
        p = C.c_void_p()
        _check(lib().maray_jit_source_refine(C.byref(self.program), C.byref(self.refine), C.byref(p)))
        try:
            return C.string_at(p).decode()
        finally:
            lib().maray_free(p)

    def arrays(self):
        """(consts, row_ops, pix_ops) as numpy copies."""
        p = self.program
        consts = np.ctypeslib.as_array(p.consts, shape=(p.n_consts,)).copy()
        row = np.ctypeslib.as_array(p.row_ops, shape=(p.n_row_ops,)).copy() if p.n_row_ops else np.zeros(0, np.uint64)
        pix = np.ctypeslib.as_array(p.pix_ops, shape=(p.n_pix_ops,)).copy() if p.n_pix_ops else np.zeros(0, np.uint64)
        return consts, row, pix


class PinnedRaster:
    """An (h, w, 3) uint8 raster in pinned host memory (maray_host_alloc): what a caller that wants the PCIe rate
    hands to the render entry points; `.array` is a numpy view of it, valid until close()."""

    def __init__(self, h, w):
        p = C.c_void_p()
        _check(lib().maray_host_alloc(h * w * 3, C.byref(p)))
        self._p = p
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(h, w, 3))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if getattr(self, '_p', None):
            self.array = None
            lib().maray_host_free(self._p)
            self._p = None

    def __del__(self):
        self.close()


class Context:
    """Device context: tape + constants + textures resident in HBM.  samples=k > 1: renders the program's raster in k x k
    blocks and writes their means (RGB8 only); every render call then takes output geometry.  filter=FILTER_TENT (needs
    samples 2, 4 or 8): the samples are reduced by a tent filter two pixels wide instead (include/maray_hip.h,
    "reconstruction filter"); filter=FILTER_CATROM (samples 2, 4 or 8; not with TRANSFER_SRGB): by a Catmull-Rom filter four
    pixels wide, whose negative lobes keep edges sharp.  transfer=TRANSFER_SRGB: box, tent and shutter average linear light,
    not bytes ("transfer")."""

    def __init__(self, tape, textures=None, device=0, backend=BACKEND_TAPE, hint_mpixels=0, samples=0, filter=FILTER_BOX,
                 transfer=TRANSFER_NONE):
        arr, n, keep = _textures(textures)
        o = CtxOpts()
        o.backend = backend
        o.hint_mpixels = hint_mpixels
        o.samples = samples
        o.filter = filter
        o.transfer = transfer
        h = C.c_void_p()
        refine = getattr(tape, 'refine', None)          # (a hand-made program has none)
        _check(lib().maray_hip_ctx_create_refined(device, C.byref(tape.program), C.byref(refine) if refine is not None else None, arr, n,
                                                  C.byref(o), C.byref(h)))
        self._h = h
        self._tape = tape

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, '_h', None):
            lib().maray_hip_ctx_free(self._h)
            self._h = None

    @property
    def param_count(self):
        n = C.c_uint32()
        _check(lib().maray_hip_ctx_param_count(self._h, C.byref(n)))
        return n.value

    def set_params(self, values):
        """The parameters' values for the launches enqueued after this call (one per parameter of the program, each
        inside its declared range).  Returns without touching the device."""
        a = (C.c_double * len(values))(*values)
        _check(lib().maray_hip_ctx_set_params(self._h, a, len(values)))

    def render_rows(self, w, h, y0, y1, want_u8=True, want_f64=True):
        rows = y1 - y0
        rgb8 = np.zeros((rows, w, 3), np.uint8) if want_u8 else None
        rgb64 = np.zeros((rows, w, 3), np.float64) if want_f64 else None
        _check(lib().maray_hip_render_rows(self._h, w, h, y0, y1, rgb8.ctypes.data if want_u8 else None,
                                           rgb64.ctypes.data if want_f64 else None))
        return rgb8, rgb64

    def render_rows_into(self, w, h, y0, y1, rgb8):
        """Rows [y0, y1) into the caller's (y1-y0, w, 3) uint8 array (pinned or pageable)."""
        assert rgb8.dtype == np.uint8 and rgb8.flags['C_CONTIGUOUS'] and rgb8.size == (y1 - y0) * w * 3
        _check(lib().maray_hip_render_rows(self._h, w, h, y0, y1, rgb8.ctypes.data, None))

    def render_tiles(self, w, h, tiles, image, on_tile=None):
        """Row ranges [(y0, y1), ...] into one (h, w, 3) uint8 raster of the whole image, pipelined (maray_hip_render_tiles)."""
        assert image.dtype == np.uint8 and image.flags['C_CONTIGUOUS'] and image.size == h * w * 3
        flat = (C.c_uint32 * (2 * len(tiles)))(*[v for t in tiles for v in t])
        cb = TILE_FN((lambda user, a, b: on_tile(a, b)) if on_tile else 0)
        _check(lib().maray_hip_render_tiles(self._h, w, h, flat, len(tiles), image.ctypes.data, cb, None))

    def _frames(self, frames):
        """(n, pointer, keep-alive) of a shutter call's frames: an (n, P) matrix of values, or an int n for a program without
        parameters (values = NULL)."""
        if isinstance(frames, (int, np.integer)):
            return int(frames), None, None
        a = np.ascontiguousarray(frames, np.float64)
        p = self.param_count
        if a.ndim != 2 or a.shape[1] != p:
            raise MarayError(-1, 'shutter frames must be an (n, %d) matrix: one column per parameter of the program' % p)
        return a.shape[0], (a.ctypes.data if a.size else None), a

    def render_rows_shutter(self, w, h, y0, y1, frames, out=None):
        """Rows [y0, y1) as the integer mean of the frames that the rows of `frames` render (maray_hip_render_rows_shutter);
        into `out`, a (y1-y0, w, 3) uint8 array, when given."""
        n, vp_, keep = self._frames(frames)
        rgb8 = np.zeros((y1 - y0, w, 3), np.uint8) if out is None else out
        assert rgb8.dtype == np.uint8 and rgb8.flags['C_CONTIGUOUS'] and rgb8.size == (y1 - y0) * w * 3
        _check(lib().maray_hip_render_rows_shutter(self._h, w, h, y0, y1, vp_, n, rgb8.ctypes.data))
        return rgb8

    def render_rows_shutter_device(self, w, h, y0, y1, frames, d_rgb8, stream=0):
        n, vp_, keep = self._frames(frames)
        _check(lib().maray_hip_render_rows_shutter_device(self._h, w, h, y0, y1, vp_, n, d_rgb8 or None, stream or None))

    def render_tiles_shutter(self, w, h, tiles, frames, image, on_tile=None):
        """render_tiles with every tile reduced from its frames on the device: one raster crosses to the host, not n."""
        assert image.dtype == np.uint8 and image.flags['C_CONTIGUOUS'] and image.size == h * w * 3
        n, vp_, keep = self._frames(frames)
        flat = (C.c_uint32 * (2 * len(tiles)))(*[v for t in tiles for v in t])
        cb = TILE_FN((lambda user, a, b: on_tile(a, b)) if on_tile else 0)
        _check(lib().maray_hip_render_tiles_shutter(self._h, w, h, flat, len(tiles), vp_, n, image.ctypes.data, cb, None))

    def render_png(self, w, h, frames=None, codes=CODES_FIXED, png_filter=PNG_FILTER_NONE, png_color=PNG_COLOR_RGB):
        """The whole w x h image as the bytes of a PNG, rendered and encoded on the device (maray_hip_render_png_opts); frames: as
        for render_rows_shutter (None: the plain render); codes=CODES_DYNAMIC: a Huffman code fitted to every band;
        png_filter=PNG_FILTER_*: the rows' PNG filter (ADAPTIVE: per row the type that makes the row smallest);
        png_color=PNG_COLOR_INDEXED / PNG_COLOR_AUTO: an indexed-colour file for at most 256 colours
        (maray_hip_render_png_color; fixed codes and filter 0 only)."""
        n, vp_, keep = (0, None, None) if frames is None else self._frames(frames)
        p, sz = C.c_void_p(), C.c_size_t()
        if png_color != PNG_COLOR_RGB:
            o = _png_color_opts(png_color, codes, png_filter, 'render_png')
            _check(lib().maray_hip_render_png_color(self._h, w, h, vp_, n, C.byref(o), C.byref(p), C.byref(sz)))
            return _take_bytes(p, sz)
        _check(lib().maray_hip_render_png_opts(self._h, w, h, vp_, n, C.byref(_png_opts(codes, png_filter)), C.byref(p), C.byref(sz)))
        return _take_bytes(p, sz)

    def render_apng(self, w, h, frames, sub=1, fps=(25, 1), loops=0):
        """n images as the bytes of one APNG, rendered and encoded on the device (maray_hip_render_apng).  frames: an
        (n * sub, P) matrix of values, image i the shutter render over its `sub` rows (sub = 1: the plain render with that row);
        or an int n for a program without parameters.  fps = (N, D) or N: every image shows for D / N seconds; loops = 0: for
        ever."""
        rows, vp_, keep = self._frames(frames)
        if sub < 1 or rows % sub:
            raise MarayError(-1, 'render_apng: frames must hold a whole number of images of %d rows' % sub)
        num, den = _delay(fps)
        p, sz = C.c_void_p(), C.c_size_t()
        _check(lib().maray_hip_render_apng(self._h, w, h, vp_, rows // sub, sub, num, den, loops, C.byref(p), C.byref(sz)))
        return _take_bytes(p, sz)

    def render_y4m(self, w, h, frames, sub=1, fps=(25, 1), sampling=YCC_420, matrix=YCC_BT601):
        """n images as the bytes of one YUV4MPEG2 file, rendered and converted to Y'CbCr planes on the device
        (maray_hip_render_y4m).  frames, sub, fps: as render_apng; sampling=YCC_444: full-resolution chroma; matrix=YCC_BT709:
        the other matrix (the file has no tag for it)."""
        rows, vp_, keep = self._frames(frames)
        if sub < 1 or rows % sub:
            raise MarayError(-1, 'render_y4m: frames must hold a whole number of images of %d rows' % sub)
        num, den = _delay(fps)
        p, sz = C.c_void_p(), C.c_size_t()
        _check(lib().maray_hip_render_y4m(self._h, w, h, vp_, rows // sub, sub, num, den, C.byref(_ycc_opts(sampling, matrix)), C.byref(p), C.byref(sz)))
        return _take_bytes(p, sz)

    def render_rows_device(self, w, h, y0, y1, d_rgb8=0, d_rgb64=0, stream=0):
        _check(lib().maray_hip_render_rows_device(self._h, w, h, y0, y1, d_rgb8 or None, d_rgb64 or None, stream or None))

    def render_blocks_device(self, w, h, y0, block_rows, block_stride, n_blocks, d_rgb8=0, d_rgb64=0, stream=0):
        """n_blocks blocks of block_rows rows, block_stride apart, first at y0, in ONE launch; outputs packed."""
        _check(lib().maray_hip_render_blocks_device(self._h, w, h, y0, block_rows, block_stride, n_blocks,
                                                    d_rgb8 or None, d_rgb64 or None, stream or None))

    def time_rows(self, w, h, y0, y1, d_rgb8=0, d_rgb64=0, reps=5):
        ms = C.c_float()
        _check(lib().maray_hip_time_rows(self._h, w, h, y0, y1, d_rgb8 or None, d_rgb64 or None, reps, C.byref(ms)))
        return ms.value

    def time_blocks(self, w, h, y0, block_rows, block_stride, n_blocks, d_rgb8=0, d_rgb64=0, reps=5):
        """time_rows for the launch render_blocks_device issues."""
        ms = C.c_float()
        _check(lib().maray_hip_time_blocks(self._h, w, h, y0, block_rows, block_stride, n_blocks, d_rgb8 or None, d_rgb64 or None,
                                           reps, C.byref(ms)))
        return ms.value

    @property
    def kernel_name(self):
        return lib().maray_hip_kernel_name(self._h).decode()

    @property
    def refine_count(self):
        """maray_jit_refine passes this context has enqueued so far (maray_hip_refine_count)."""
        n = C.c_uint64()
        _check(lib().maray_hip_refine_count(self._h, C.byref(n)))
        return n.value

    @property
    def census_count(self):
        """maray_jit_census launches this context has enqueued so far (maray_hip_census_count)."""
        n = C.c_uint64()
        _check(lib().maray_hip_census_count(self._h, C.byref(n)))
        return n.value

    @property
    def cover_count(self):
        """maray_jit_cover launches this context has enqueued so far (maray_hip_cover_count)."""
        n = C.c_uint64()
        _check(lib().maray_hip_cover_count(self._h, C.byref(n)))
        return n.value

    def debug_cover_words(self):
        """Test access (maray_hip_debug_cover_words): like debug_census_words(); where the last launch ran maray_jit_pixels_cov, the
        words with cover bits that it read."""
        n, per = C.c_size_t(), C.c_uint32()
        _check(lib().maray_hip_debug_cover_words(self._h, None, 0, C.byref(n), C.byref(per)))
        out = np.zeros(n.value, np.uint64)
        _check(lib().maray_hip_debug_cover_words(self._h, out.ctypes.data, n.value, C.byref(n), C.byref(per)))
        return out.reshape(-1, per.value)

    @property
    def rowscan_count(self):
        """maray_jit_rowscan launches this context has enqueued so far (maray_hip_rowscan_count)."""
        n = C.c_uint64()
        _check(lib().maray_hip_rowscan_count(self._h, C.byref(n)))
        return n.value

    @property
    def prepass_count(self):
        """Launches of maray_jit_pixels_pp this context has enqueued so far (maray_hip_prepass_count)."""
        n = C.c_uint64()
        _check(lib().maray_hip_prepass_count(self._h, C.byref(n)))
        return n.value

    @property
    def deferred_count(self):
        """Tiles the most recent launch deferred to the interpreter (maray_hip_deferred_count); waits for the context's work."""
        n = C.c_uint64()
        _check(lib().maray_hip_deferred_count(self._h, C.byref(n)))
        return n.value

    def debug_row_words(self):
        """Test access (maray_hip_debug_row_words): of the set the last launch used, (xbits, rwords, used): the fourth table of
        guard words, (rectangles, words per rectangle) uint64 with the row flags; the row words, (rows x rectangles per row, words
        per rectangle), of which only the flagged rectangles' are meaningful; whether that launch ran maray_jit_pixels_rw.
        Both arrays are empty for a set that has been through no row scan."""
        nx, nr, per, used = C.c_size_t(), C.c_size_t(), C.c_uint32(), C.c_int()
        _check(lib().maray_hip_debug_row_words(self._h, None, 0, C.byref(nx), None, 0, C.byref(nr), C.byref(per), C.byref(used)))
        xb, rw = np.zeros(nx.value, np.uint64), np.zeros(nr.value, np.uint64)
        _check(lib().maray_hip_debug_row_words(self._h, xb.ctypes.data, nx.value, C.byref(nx), rw.ctypes.data, nr.value, C.byref(nr), C.byref(per), C.byref(used)))
        return xb.reshape(-1, per.value), rw.reshape(-1, per.value), bool(used.value)

    def debug_row_sets(self):
        """Test access (maray_hip_debug_row_sets): (set, kept_sets, kept_bytes, budget, held_bytes) of a MARAY_BACKEND_JIT context:
        the set of ROW tables the last launch used (0 = the scratch, -1 before any launch), how many sets are kept, the bytes
        accounted to them, their budget, and the device bytes the kept sets' tables hold.  Waits for nothing."""
        s, n = C.c_int32(), C.c_uint32()
        kept, budget, held = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().maray_hip_debug_row_sets(self._h, C.byref(s), C.byref(n), C.byref(kept), C.byref(budget), C.byref(held)))
        return s.value, n.value, kept.value, budget.value, held.value

    def debug_guard_words(self):
        """Test access (maray_hip_debug_guard_words): the guard words of the set the last launch used, (rectangles, words per
        rectangle) uint64, the rectangles of a group of rows adjacent."""
        n, per = C.c_size_t(), C.c_uint32()
        _check(lib().maray_hip_debug_guard_words(self._h, None, 0, C.byref(n), C.byref(per)))
        out = np.zeros(n.value, np.uint64)
        _check(lib().maray_hip_debug_guard_words(self._h, out.ctypes.data, n.value, C.byref(n), C.byref(per)))
        return out.reshape(-1, per.value)

    def debug_census_words(self):
        """Test access (maray_hip_debug_census_words): the guard words the last launch read, shaped like debug_guard_words():
        those, until the set has been through its census; then what the census left of them."""
        n, per = C.c_size_t(), C.c_uint32()
        _check(lib().maray_hip_debug_census_words(self._h, None, 0, C.byref(n), C.byref(per)))
        out = np.zeros(n.value, np.uint64)
        _check(lib().maray_hip_debug_census_words(self._h, out.ctypes.data, n.value, C.byref(n), C.byref(per)))
        return out.reshape(-1, per.value)

    @property
    def launch_counts(self):
        """(ROW passes, launch-order kernels) this context has enqueued so far (maray_hip_launch_counts)."""
        rows, order = C.c_uint64(), C.c_uint64()
        _check(lib().maray_hip_launch_counts(self._h, C.byref(rows), C.byref(order)))
        return rows.value, order.value


def gen_to_image(scene, size=None, textures=None, backend=BACKEND_AUTO, n_devices=0, tile_rows=0, report=None,
                 report_kind=REPORT_NONE, report_value=0, out=None, samples=0, params=None, shutter=0, spans=None, filter=FILTER_BOX,
                 transfer=TRANSFER_NONE):
    """`gen_to_image` (src/lib.rs:1177-1195) with RenderMethod::Hip → HxWx3 uint8 (into `out` when given).
    samples=k: anti-aliased, k x k samples per pixel averaged (include/maray_hip.h, supersampling); filter=FILTER_TENT: reduced
    by a tent filter two pixels wide instead of the box (needs samples 2, 4 or 8); filter=FILTER_CATROM: by a Catmull-Rom
    filter four pixels wide (samples 2, 4 or 8; not with transfer=TRANSFER_SRGB).
    params={name_or_id: value}: sets these declared parameters of the scene first (Scene.declare_param); the scene's
    program and contexts are found again whatever the values.
    shutter=n, spans={name_or_id: span}: motion blur, the integer mean of n frames whose parameters cover their spans around
    the values (Scene.shutter_values), averaged on the device; spans are set on the scene first, like params.
    transfer=TRANSFER_SRGB: samples and frames are averaged in linear light (include/maray_hip.h, "transfer")."""
    for k, v in (params or {}).items():
        scene.set_param(scene.param_index(k), v)
    for k, v in (spans or {}).items():
        scene.set_param_span(scene.param_index(k), v)
    w, h = size if size else scene.size
    img = np.zeros((h, w, 3), np.uint8) if out is None else out
    assert img.shape == (h, w, 3) and img.dtype == np.uint8 and img.flags['C_CONTIGUOUS']
    arr, n, keep = _textures(textures)
    go = GenOpts()
    go.backend, go.n_devices, go.tile_rows, go.samples, go.shutter, go.filter = backend, n_devices, tile_rows, samples, shutter, filter
    go.transfer = transfer

    def _cb(user, p, cw, ch, progress):
        if report:
            report(img, progress)
    cb = REPORT_FN(_cb)
    _check(lib().maray_gen_to_image(scene._h, arr, n, C.byref(go), Report(report_kind, report_value), cb, None,
                                    img.ctypes.data, w, h))
    return img


def gen(scene, path, textures=None, backend=BACKEND_AUTO, n_devices=0, report_kind=REPORT_NONE, report_value=0, samples=0, shutter=0, filter=FILTER_BOX,
        encoder=ENCODER_HOST, transfer=TRANSFER_NONE):
    """`gen` (src/lib.rs:1199-1213): render and write a PNG (samples=k: anti-aliased; shutter=n: motion blur over the scene's
    parameter spans; filter=FILTER_TENT / FILTER_CATROM: the tent / Catmull-Rom reconstruction filter; transfer=TRANSFER_SRGB: averaged in linear light; as
    gen_to_image).  encoder=ENCODER_DEVICE: the PNG's
    zlib stream is built on the devices and no raster crosses to the host (include/maray_hip.h, "device PNG encoder");
    ENCODER_DEVICE | ENCODER_DYNAMIC: with dynamic-Huffman codes, the same pixels in a smaller file."""
    arr, n, keep = _textures(textures)
    go = GenOpts()
    go.backend, go.n_devices, go.samples, go.shutter, go.filter, go.encoder = backend, n_devices, samples, shutter, filter, encoder
    go.transfer = transfer
    _check(lib().maray_gen(scene._h, arr, n, C.byref(go), Report(report_kind, report_value), os.fsencode(path)))


def _delay(fps):
    """(delay_num, delay_den) of fps = N or (N, D): D / N seconds an image."""
    n, d = fps if isinstance(fps, (tuple, list)) else (fps, 1)
    return int(d), int(n)


def gen_animation(scene, path, frames, fps=(25, 1), loops=0, textures=None, backend=BACKEND_AUTO, n_devices=0, samples=0, shutter=0, spans=None,
                  filter=FILTER_BOX, transfer=TRANSFER_NONE, codes=CODES_FIXED, container=CONTAINER_APNG, sampling=YCC_420, matrix=YCC_BT601):
    """An animation of the scene as one APNG at `path`, rendered and encoded on one device (maray_gen_animation_ex;
    container=CONTAINER_Y4M: as one YUV4MPEG2 file of Y'CbCr planes converted on the device and streamed to `path` frame by
    frame, with sampling=YCC_* and matrix=YCC_*; loops and codes mean nothing there).  frames: an
    (n, P) matrix, one row of values per image and one column per declared parameter, or a dict {name_or_id: sequence} -- the
    parameters it does not name keep their current value.  fps, loops: as Context.render_apng; the other options as gen's
    (shutter=n with spans: every image the mean of n sub-frames around its values); codes=CODES_DYNAMIC: dynamic-Huffman
    codes for every frame (the flag ENCODER_DYNAMIC on the options' encoder word).  The scene's values are as they were
    afterwards."""
    for k, v in (spans or {}).items():
        scene.set_param_span(scene.param_index(k), v)
    P = scene.param_count
    if isinstance(frames, dict):
        lengths = {len(v) for v in frames.values()}
        if len(lengths) != 1:
            raise MarayError(-1, 'gen_animation: the sequences of `frames` must be equally long')
        a = np.empty((lengths.pop(), P), np.float64)
        for p in range(P):
            a[:, p] = scene.param_info(p)[3]
        for k, v in frames.items():
            a[:, scene.param_index(k)] = np.asarray(v, np.float64)
    else:
        a = np.ascontiguousarray(frames, np.float64)
        if a.ndim != 2 or a.shape[1] != P:
            raise MarayError(-1, 'gen_animation: frames must be an (n, %d) matrix: one column per declared parameter' % P)
    arr, n, keep = _textures(textures)
    go = GenOpts()
    go.backend, go.n_devices, go.samples, go.shutter, go.filter, go.transfer = backend, n_devices, samples, shutter, filter, transfer
    if codes not in (CODES_FIXED, CODES_DYNAMIC):
        raise MarayError(-1, 'gen_animation: unknown PNG codes')
    go.encoder = ENCODER_DYNAMIC if codes == CODES_DYNAMIC else 0
    num, den = _delay(fps)
    ao = AnimOpts()
    ao.container, ao.sampling, ao.matrix = container, sampling, matrix
    _check(lib().maray_gen_animation_ex(scene._h, arr, n, C.byref(go), a.ctypes.data if a.size else None, a.shape[0], num, den, loops, C.byref(ao),
                                        os.fsencode(path)))


def frame_delta(d_prev, d_cur, w, h, device=0, stream=0):
    """(x0, y0, x1, y1): the half-open bounding box of the pixels in which two packed (h, w, 3) uint8 rasters in device memory
    (any alignment) differ, (0, 0, 0, 0) when none does (maray_hip_frame_delta); enqueued on `stream` and waited for."""
    box = (C.c_uint32 * 4)()
    _check(lib().maray_hip_frame_delta(device, d_prev or None, d_cur or None, w, h, stream or None, box))
    return tuple(box)


def apng_encode_device(d_frames, n, w, h, fps=(25, 1), loops=0, device=0, stream=0):
    """n packed (h, w, 3) uint8 frames, 3 w h bytes apart in device memory (any alignment) -> the bytes of an APNG, encoded on
    the device (maray_hip_apng_encode_device); enqueued on `stream` and waited for."""
    num, den = _delay(fps)
    p, sz = C.c_void_p(), C.c_size_t()
    _check(lib().maray_hip_apng_encode_device(device, d_frames or None, n, w, h, num, den, loops, stream or None, C.byref(p), C.byref(sz)))
    return _take_bytes(p, sz)


def time_frame_delta(w, h, device=0, reps=10, with_copy=False):
    """Average ms of the frame-delta kernels over two w x h rasters (maray_hip_time_frame_delta); with_copy: (that, the
    average ms of a device-to-device copy of one raster's bytes timed in the same call)."""
    ms, cp = C.c_float(), C.c_float()
    if not with_copy:
        _check(lib().maray_hip_time_frame_delta(device, w, h, reps, C.byref(ms)))
        return ms.value
    _check(lib().maray_hip_time_frame_delta_copy(device, w, h, reps, C.byref(ms), C.byref(cp)))
    return ms.value, cp.value


def ycc_frame_bytes(w, h, sampling=YCC_420):
    """Bytes of one frame's Y', Cb and Cr planes (maray_ycc_frame_bytes); needs no device."""
    n = C.c_size_t()
    _check(lib().maray_ycc_frame_bytes(w, h, sampling, C.byref(n)))
    return n.value


def rgb_to_ycc(d_rgb8, w, h, d_planes, sampling=YCC_420, matrix=YCC_BT601, device=0, stream=0):
    """A packed (h, w, 3) uint8 raster in device memory -> ycc_frame_bytes(w, h, sampling) bytes at d_planes: the Y', Cb and Cr
    planes one after the other (maray_hip_rgb_to_ycc; both at any alignment).  Enqueued on `stream`: it does not synchronise."""
    _check(lib().maray_hip_rgb_to_ycc(device, d_rgb8 or None, w, h, C.byref(_ycc_opts(sampling, matrix)), d_planes or None, stream or None))


def y4m_encode_device(d_frames, n, w, h, fps=(25, 1), sampling=YCC_420, matrix=YCC_BT601, device=0, stream=0):
    """n packed (h, w, 3) uint8 frames, 3 w h bytes apart in device memory (any alignment) -> the bytes of a YUV4MPEG2 file,
    converted on the device (maray_hip_y4m_encode_device); the conversions are enqueued on `stream` and waited for."""
    num, den = _delay(fps)
    p, sz = C.c_void_p(), C.c_size_t()
    _check(lib().maray_hip_y4m_encode_device(device, d_frames or None, n, w, h, num, den, C.byref(_ycc_opts(sampling, matrix)), stream or None,
                                             C.byref(p), C.byref(sz)))
    return _take_bytes(p, sz)


def time_rgb_to_ycc(w, h, sampling=YCC_420, matrix=YCC_BT601, device=0, reps=10):
    """(average ms of the conversion kernel over a w x h raster, average ms of a device-to-device copy that moves as many bytes,
    timed in the same call) (maray_hip_time_rgb_to_ycc)."""
    ms, cp = C.c_float(), C.c_float()
    _check(lib().maray_hip_time_rgb_to_ycc(device, w, h, C.byref(_ycc_opts(sampling, matrix)), reps, C.byref(ms), C.byref(cp)))
    return ms.value, cp.value


def _take_bytes(p, sz):
    try:
        return C.string_at(p, sz.value)
    finally:
        lib().maray_free(p)


def png_encode_device(d_ptr, w, h, device=0, stream=0, codes=CODES_FIXED, png_filter=PNG_FILTER_NONE, png_color=PNG_COLOR_RGB):
    """A packed (h, w, 3) uint8 raster in device memory (any alignment) -> the bytes of a PNG, encoded on the device
    (maray_hip_png_encode_device_opts); enqueued on `stream` and waited for.  codes=CODES_DYNAMIC: a Huffman code fitted to
    every band of rows instead of the fixed codes; png_filter=PNG_FILTER_*: the rows' PNG filter; png_color=PNG_COLOR_INDEXED /
    PNG_COLOR_AUTO: an indexed-colour file for at most 256 colours (maray_hip_png_encode_device_color; fixed codes, filter 0)."""
    p, sz = C.c_void_p(), C.c_size_t()
    if png_color != PNG_COLOR_RGB:
        o = _png_color_opts(png_color, codes, png_filter, 'png_encode_device')
        _check(lib().maray_hip_png_encode_device_color(device, d_ptr or None, w, h, C.byref(o), stream or None, C.byref(p), C.byref(sz)))
        return _take_bytes(p, sz)
    _check(lib().maray_hip_png_encode_device_opts(device, d_ptr or None, w, h, C.byref(_png_opts(codes, png_filter)), stream or None, C.byref(p),
                                                  C.byref(sz)))
    return _take_bytes(p, sz)


def time_png_encode(d_ptr, w, h, device=0, reps=10, codes=CODES_FIXED, png_filter=PNG_FILTER_NONE, png_color=PNG_COLOR_RGB):
    """(average ms of the encoder's kernels over the raster as one band, bytes of the stream they make); with a png_filter the
    kernels that choose the rows' types are among them; with a png_color mode the kernels that collect the colours
    (maray_hip_time_png_encode_color)."""
    ms, nb = C.c_float(), C.c_uint64()
    if png_color != PNG_COLOR_RGB:
        o = _png_color_opts(png_color, codes, png_filter, 'time_png_encode')
        _check(lib().maray_hip_time_png_encode_color(device, d_ptr or None, w, h, C.byref(o), reps, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value
    _check(lib().maray_hip_time_png_encode_opts(device, d_ptr or None, w, h, C.byref(_png_opts(codes, png_filter)), reps, C.byref(ms), C.byref(nb)))
    return ms.value, nb.value


def png_palette(d_ptr, w, h, device=0, stream=0):
    """The distinct colours of a packed (h, w, 3) uint8 raster in device memory, collected on the device (maray_hip_png_palette):
    (n, uint8[n, 3]) in ascending order of R * 65536 + G * 256 + B, or (257, an empty array) for more than 256 colours."""
    n, pal = C.c_uint32(), np.zeros((256, 3), np.uint8)
    _check(lib().maray_hip_png_palette(device, d_ptr or None, w, h, stream or None, C.byref(n), pal.ctypes.data))
    return n.value, pal[:n.value if n.value <= 256 else 0].copy()


def png_dynamic_codes(lit_counts, dist_counts):
    """The host's part of the dynamic coder (maray_png_dynamic_codes; no device): 286 literal/length counts and 30 distance
    counts -> (lit_lens uint8[286], dist_lens uint8[30], the block header's bytes, its bits)."""
    lit = np.ascontiguousarray(lit_counts, np.uint32)
    dist = np.ascontiguousarray(dist_counts, np.uint32)
    if lit.shape != (286,) or dist.shape != (30,):
        raise MarayError(-1, 'png_dynamic_codes: 286 literal/length counts and 30 distance counts')
    lit_lens, dist_lens, header, bits = np.zeros(286, np.uint8), np.zeros(30, np.uint8), np.zeros(512, np.uint8), C.c_size_t()
    _check(lib().maray_png_dynamic_codes(lit.ctypes.data, dist.ctypes.data, lit_lens.ctypes.data, dist_lens.ctypes.data, header.ctypes.data,
                                         header.size, C.byref(bits)))
    return lit_lens, dist_lens, header[:(bits.value + 7) // 8].tobytes(), bits.value


def png_bytes_to_host():
    """Bytes the device encoders of this process have copied to the host so far."""
    return lib().maray_hip_png_bytes_to_host()


def time_filter(w, rows, k, device=0, reps=10, filter=FILTER_TENT, transfer=TRANSFER_NONE):
    """Average ms of maray_filter_tent<k> alone over a w x rows output image (maray_hip_time_filter); with
    transfer=TRANSFER_SRGB of maray_filter_tent_lin<k> or, filter=FILTER_BOX, maray_filter_box_lin<k>; with filter=FILTER_CATROM
    of maray_filter_catrom<k> (maray_hip_time_filter_ex)."""
    ms = C.c_float()
    if filter == FILTER_TENT and transfer == TRANSFER_NONE:
        _check(lib().maray_hip_time_filter(device, w, rows, k, reps, C.byref(ms)))
    else:
        _check(lib().maray_hip_time_filter_ex(device, w, rows, k, filter, transfer, reps, C.byref(ms)))
    return ms.value


def time_shutter_reduce(nbytes, n, device=0, reps=10, transfer=TRANSFER_NONE):
    """Average ms of the passes that reduce n frames of nbytes bytes: maray_shutter_reduce, or with transfer=TRANSFER_SRGB
    maray_shutter_reduce_lin (maray_hip_time_shutter_reduce_ex)."""
    ms = C.c_float()
    _check(lib().maray_hip_time_shutter_reduce_ex(device, nbytes, n, transfer, reps, C.byref(ms)))
    return ms.value


def transfer_table(transfer=TRANSFER_SRGB):
    """(decode D[256], thresholds T[256]) of a transfer as uint16 arrays (maray_transfer_table; T[0] = 0); needs no device."""
    d, t = np.zeros(256, np.uint16), np.zeros(256, np.uint16)
    _check(lib().maray_transfer_table(transfer, d.ctypes.data, t.ctypes.data))
    return d, t


def gen_cache_clear():
    """Frees the tapes and contexts maray_gen_to_image keeps between calls."""
    lib().maray_gen_cache_clear()


def gen_cache_info():
    """One line per idle context maray_gen_to_image keeps: program key, device, kernel, the size it was chosen for."""
    buf = C.create_string_buffer(1 << 16)
    _check(lib().maray_gen_cache_info(buf, len(buf)))
    return buf.value.decode().splitlines()


def png_write(path, rgb8):
    a = np.ascontiguousarray(rgb8, np.uint8)
    _check(lib().maray_png_write(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]))


def image_read(path):
    """`image::open(path).to_rgb8()`: a texture file in any format the library reads -> HxWx3 uint8."""
    return png_read(path, _fn='maray_image_read')


def png_read(path, _fn='maray_png_read'):
    p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
    _check(getattr(lib(), _fn)(os.fsencode(path), C.byref(p), C.byref(w), C.byref(h)))
    try:
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(h.value, w.value, 3)).copy()
    finally:
        lib().maray_free(p)
    return a
