"""maray_amd — MI355X (gfx950) per-pixel expression evaluator for maray scenes.

A thin ctypes binding over libmaray_hip.so (C ABI in include/maray_hip.h).
The compute path is the HIP library; there is no Python or CPU fallback: every
render call raises MarayError when the library or a gfx950 device is missing.
"""
from .api import (BACKEND_AUTO, BACKEND_JIT, BACKEND_TAPE, BACKEND_TAPE_SMEM, ENCODER_DEVICE, ENCODER_HOST, FILTER_BOX, FILTER_CATROM, FILTER_TENT, TRANSFER_NONE, TRANSFER_SRGB, Context, CtxOpts, GenOpts, MarayError, PinnedRaster, Program, Scene, Tape, device_count, gen,
                  gen_cache_clear, gen_cache_info, gen_to_image, image_read, lib, lib_path, png_bytes_to_host, png_encode_device, png_read, png_write, time_filter,
                  time_png_encode, time_shutter_reduce, transfer_table, var_id, version,
                  apng_encode_device, frame_delta, gen_animation, time_frame_delta,
                  CODES_DYNAMIC, CODES_FIXED, ENCODER_DYNAMIC, png_dynamic_codes,
                  PNG_FILTER_ADAPTIVE, PNG_FILTER_AVERAGE, PNG_FILTER_NONE, PNG_FILTER_PAETH, PNG_FILTER_SUB, PNG_FILTER_UP, PngOpts,
                  PNG_COLOR_AUTO, PNG_COLOR_INDEXED, PNG_COLOR_RGB, PngColorOpts, png_palette,
                  CONTAINER_APNG, CONTAINER_Y4M, YCC_420, YCC_444, YCC_BT601, YCC_BT709, AnimOpts, YccOpts, rgb_to_ycc, time_rgb_to_ycc, y4m_encode_device,
                  ycc_frame_bytes)

__all__ = ['Scene', 'Tape', 'Context', 'PinnedRaster', 'MarayError', 'gen', 'gen_to_image', 'gen_cache_clear', 'gen_cache_info', 'device_count', 'lib', 'lib_path',
           'png_read', 'png_write', 'image_read', 'version', 'var_id', 'Program', 'BACKEND_TAPE', 'BACKEND_TAPE_SMEM', 'BACKEND_JIT', 'BACKEND_AUTO', 'FILTER_BOX', 'FILTER_TENT', 'FILTER_CATROM',
           'time_filter', 'ENCODER_HOST', 'ENCODER_DEVICE', 'GenOpts', 'png_encode_device', 'time_png_encode', 'png_bytes_to_host',
           'TRANSFER_NONE', 'TRANSFER_SRGB', 'CtxOpts', 'transfer_table', 'time_shutter_reduce',
           'frame_delta', 'apng_encode_device', 'gen_animation', 'time_frame_delta',
           'CODES_FIXED', 'CODES_DYNAMIC', 'ENCODER_DYNAMIC', 'png_dynamic_codes',
           'PNG_FILTER_NONE', 'PNG_FILTER_ADAPTIVE', 'PNG_FILTER_SUB', 'PNG_FILTER_UP', 'PNG_FILTER_AVERAGE', 'PNG_FILTER_PAETH', 'PngOpts',
           'PNG_COLOR_RGB', 'PNG_COLOR_INDEXED', 'PNG_COLOR_AUTO', 'PngColorOpts', 'png_palette',
           'YCC_420', 'YCC_444', 'YCC_BT601', 'YCC_BT709', 'CONTAINER_APNG', 'CONTAINER_Y4M', 'YccOpts', 'AnimOpts', 'ycc_frame_bytes', 'rgb_to_ycc',
           'y4m_encode_device', 'time_rgb_to_ycc']
