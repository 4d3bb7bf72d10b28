"""ctypes binding of the product library rawspeed_amd/librsx.so (include/rsx.h).

The library is the product; this module only marshals arguments.  Loading fails
loudly if the library is missing, and every decode entry point fails with
RSX_ERR_DEVICE when there is no GPU -- there is no CPU fallback anywhere.
"""
import ctypes as C
import os

import numpy as np

from . import abi, build

_lib = None

# every symbol include/rsx.h declares (tests check that all of them resolve)
EXPORTS = [
    "rsx_abi_version", "rsx_status_string", "rsx_device_count", "rsx_ctx_create",
    "rsx_ctx_destroy", "rsx_ctx_last_error", "rsx_ctx_host_calls", "rsx_ctx_chunked_calls",
    "rsx_host_alloc", "rsx_host_free", "rsx_host_register", "rsx_host_unregister",
    "rsx_unpack_validate", "rsx_unpack_u16",
    "rsx_unpack_f32_validate", "rsx_unpack_f32", "rsx_unpack_f32_plan_create",
    "rsx_unpack_variant_validate", "rsx_unpack_variant_u16", "rsx_unpack_variant_plan_create",
    "rsx_ljpeg_validate", "rsx_ljpeg_decode",
    "rsx_cr2_validate", "rsx_cr2_decode",
    "rsx_sraw_validate", "rsx_sraw_interpolate", "rsx_sraw_plan_create",
    "rsx_nikon_validate", "rsx_nikon_decompress", "rsx_nikon_plan_create",
    "rsx_pentax_validate", "rsx_pentax_decompress", "rsx_pentax_plan_create",
    "rsx_hasselblad_validate", "rsx_hasselblad_decompress", "rsx_hasselblad_plan_create",
    "rsx_samsung_v1_validate", "rsx_samsung_v1_decompress", "rsx_samsung_v1_plan_create",
    "rsx_samsung_v2_validate", "rsx_samsung_v2_decompress", "rsx_samsung_v2_plan_create",
    "rsx_sony_arw1_validate", "rsx_sony_arw1_decompress", "rsx_sony_arw1_plan_create",
    "rsx_phase_one_validate", "rsx_phase_one_decompress", "rsx_phase_one_plan_create",
    "rsx_sony_arw2_validate", "rsx_sony_arw2_decompress", "rsx_sony_arw2_plan_create",
    "rsx_panasonic_validate", "rsx_panasonic_decompress", "rsx_panasonic_plan_create",
    "rsx_samsung_v0_validate", "rsx_samsung_v0_decompress", "rsx_samsung_v0_plan_create",
    "rsx_panasonic_v4_validate", "rsx_panasonic_v4_decompress", "rsx_panasonic_v4_plan_create",
    "rsx_panasonic_v4_plan_bad_pixels",
    "rsx_nikon_snef_validate", "rsx_nikon_snef_decompress", "rsx_nikon_snef_plan_create",
    "rsx_vc5_validate", "rsx_vc5_decompress", "rsx_vc5_plan_create", "rsx_vc5_plan_bands",
    "rsx_iiq_correct_validate", "rsx_iiq_correct", "rsx_phase_one_decompress_corrected",
    "rsx_iiq_correct_plan_create", "rsx_iiq_defect_positions", "rsx_phase_one_decompress_fixed",
    "rsx_dng_post_validate", "rsx_dng_post", "rsx_dng_decompress_ljpeg_post",
    "rsx_dng_decompress_uncompressed_post", "rsx_dng_post_plan_create",
    "rsx_dng_post_plan_result", "rsx_dng_post_plan_bad_pixels",
    "rsx_bad_pixels_validate", "rsx_bad_pixels_fix", "rsx_panasonic_v4_decompress_fixed",
    "rsx_bad_pixels_plan_create", "rsx_bad_pixels_plan_result",
    "rsx_scale_validate", "rsx_scale_black_white", "rsx_scale_plan_create", "rsx_scale_plan_result",
    "rsx_dng_finish", "rsx_dng_decompress_ljpeg_finish", "rsx_dng_decompress_uncompressed_finish",
    "rsx_dng_decompress_ljpeg", "rsx_dng_decompress_uncompressed",
    "rsx_dng_deflate_validate", "rsx_dng_decompress_deflate", "rsx_dng_deflate_plan_create",
    "rsx_dng_jpeg_validate", "rsx_dng_decompress_jpeg", "rsx_dng_jpeg_plan_create",
    "rsx_dng_jpeg_plan_tile_status",
    "rsx_dng_lossy_validate", "rsx_dng_lossy_decompress",
    "rsx_fuji_parse", "rsx_fuji_validate", "rsx_fuji_decompress", "rsx_fuji_plan_create",
    "rsx_fuji_plan_strip_status",
    "rsx_olympus_validate", "rsx_olympus_decompress", "rsx_olympus_plan_create",
    "rsx_olympus_plan_job_status",
    "rsx_kodak_validate", "rsx_kodak_decompress", "rsx_kodak_plan_create",
    "rsx_crw_validate", "rsx_crw_decompress", "rsx_crw_plan_create", "rsx_crw_plan_stats",
    "rsx_raf_rotate_geometry", "rsx_raf_rotate_validate", "rsx_raf_rotate",
    "rsx_raf_rotate_plan_create",
    "rsx_sony_decrypt", "rsx_sony_srf_validate", "rsx_sony_srf_decompress",
    "rsx_sony_srf_plan_create",
    "rsx_image_hash_validate", "rsx_image_hash", "rsx_image_hash_plan_create",
    "rsx_encode_pack_validate", "rsx_encode_pack_u16", "rsx_encode_pack_plan_create",
    "rsx_encode_ljpeg_validate", "rsx_encode_ljpeg_bound", "rsx_encode_ljpeg",
    "rsx_encode_ljpeg_plan_create", "rsx_encode_ljpeg_plan_result", "rsx_encode_ljpeg_container",
    "rsx_encode_ljpeg_histogram", "rsx_encode_huff_from_histogram",
    "rsx_fpwrite_fit", "rsx_fpwrite_pack_validate", "rsx_fpwrite_pack",
    "rsx_fpwrite_pack_plan_create", "rsx_fpwrite_pack_plan_result",
    "rsx_fpwrite_deflate_validate", "rsx_fpwrite_deflate_bound", "rsx_fpwrite_deflate",
    "rsx_fpwrite_deflate_plan_create", "rsx_fpwrite_deflate_plan_result",
    "rsx_dctwrite_quality_tables", "rsx_dctwrite_validate", "rsx_dctwrite_bound", "rsx_dctwrite",
    "rsx_dctwrite_plan_create", "rsx_dctwrite_plan_result",
    "rsx_unpack_plan_create", "rsx_ljpeg_plan_create", "rsx_cr2_plan_create",
    "rsx_plan_run", "rsx_plan_results", "rsx_plan_set_timing",
    "rsx_plan_kernel_time", "rsx_plan_kernel_table", "rsx_plan_destroy", "rsx_probe_stream_copy",
]


class RsxError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        super().__init__("%s (%d) %s" % (abi.STATUS_NAMES.get(status, "?"), status, what))


def lib():
    global _lib
    if _lib is None:
        # RSX_LIB: A/B experiments with alternative builds of the same library
        path = os.environ.get("RSX_LIB") or build.LIB_CORE
        if not os.path.exists(path):
            raise RuntimeError(
                "rawspeed_amd/librsx.so is not built: run `python -m rawspeed_amd.build` "
                "(or __graft_entry__.build()); there is no fallback implementation")
        # PyTorch bundles its own libamdhip64; two HIP runtimes in one process do
        # not coexist ("No HIP GPUs are available").  Loading torch's first makes
        # librsx.so's DT_NEEDED libamdhip64 resolve to the same, single runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        L.rsx_status_string.restype = C.c_char_p
        L.rsx_ctx_last_error.restype = C.c_char_p
        L.rsx_ctx_last_error.argtypes = [C.c_void_p]
        L.rsx_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.rsx_ctx_destroy.argtypes = [C.c_void_p]
        L.rsx_unpack_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_ljpeg_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_cr2_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_unpack_u16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]
        L.rsx_unpack_f32_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_unpack_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]
        L.rsx_unpack_variant_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_unpack_variant_u16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_size_t, C.c_void_p]
        L.rsx_ljpeg_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_void_p]
        L.rsx_cr2_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p]
        L.rsx_sraw_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_sraw_interpolate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_nikon_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_pentax_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_hasselblad_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_hasselblad_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_void_p, C.c_void_p]
        L.rsx_sony_arw1_validate.argtypes = [C.c_void_p]
        L.rsx_sony_arw1_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p]
        L.rsx_samsung_v1_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_phase_one_validate.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_phase_one_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_sony_arw2_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_sony_arw2_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_void_p]
        L.rsx_panasonic_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_panasonic_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p]
        L.rsx_panasonic_v4_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_panasonic_v4_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rsx_panasonic_v4_plan_bad_pixels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32,
                                                       C.c_void_p]
        L.rsx_nikon_snef_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_nikon_snef_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p]
        L.rsx_vc5_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_vc5_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_iiq_correct_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_iiq_correct.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_phase_one_decompress_corrected.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]
        L.rsx_iiq_defect_positions.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p,
                                               C.c_uint32, C.c_void_p]
        L.rsx_phase_one_decompress_fixed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_uint32,
                                                      C.c_void_p]
        L.rsx_dng_post_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint32]
        L.rsx_dng_post.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_uint32]
        L.rsx_dng_decompress_ljpeg_post.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_uint32]
        L.rsx_dng_decompress_uncompressed_post.argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_uint32]
        L.rsx_dng_post_plan_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_dng_post_plan_bad_pixels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32,
                                                   C.c_void_p]
        L.rsx_bad_pixels_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_bad_pixels_fix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_panasonic_v4_decompress_fixed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_size_t, C.c_void_p, C.c_void_p,
                                                        C.c_uint32, C.c_void_p]
        L.rsx_bad_pixels_plan_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_scale_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_scale_black_white.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_scale_plan_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_dng_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint32, C.c_void_p]
        L.rsx_dng_decompress_ljpeg_finish.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_uint32,
                                                      C.c_void_p]
        L.rsx_dng_decompress_uncompressed_finish.argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_uint32,
                                                             C.c_void_p]
        L.rsx_vc5_plan_bands.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_samsung_v0_validate.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        L.rsx_samsung_v0_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p]
        L.rsx_dng_deflate_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_dng_decompress_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        L.rsx_dng_jpeg_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_dng_decompress_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        L.rsx_dng_jpeg_plan_tile_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_dng_lossy_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint32]
        L.rsx_dng_lossy_decompress.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_uint32, C.c_void_p]
        L.rsx_fuji_parse.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_fuji_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_fuji_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_void_p]
        L.rsx_fuji_plan_strip_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_olympus_validate.argtypes = [C.c_size_t, C.c_void_p]
        L.rsx_olympus_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_olympus_plan_job_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_kodak_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_kodak_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]
        L.rsx_crw_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        L.rsx_crw_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_crw_plan_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_raf_rotate_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_raf_rotate_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_raf_rotate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_sony_decrypt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32]
        L.rsx_sony_srf_validate.argtypes = [C.c_size_t, C.c_void_p]
        L.rsx_sony_srf_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                              C.c_void_p]
        L.rsx_image_hash_validate.argtypes = [C.c_void_p, C.c_int32]
        L.rsx_image_hash.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.rsx_encode_pack_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_encode_pack_u16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]
        L.rsx_encode_ljpeg_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_encode_ljpeg_bound.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_encode_ljpeg_bound.restype = C.c_uint64
        L.rsx_encode_ljpeg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_size_t, C.c_void_p]
        L.rsx_encode_ljpeg_plan_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_encode_ljpeg_container.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsx_encode_ljpeg_histogram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_encode_huff_from_histogram.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.rsx_fpwrite_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rsx_fpwrite_pack_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsx_fpwrite_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p]
        L.rsx_fpwrite_pack_plan_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_fpwrite_deflate_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_fpwrite_deflate_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_fpwrite_deflate_bound.restype = C.c_uint64
        L.rsx_fpwrite_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        L.rsx_fpwrite_deflate_plan_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_dctwrite_quality_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.rsx_dctwrite_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_dctwrite_bound.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_dctwrite_bound.restype = C.c_uint64
        L.rsx_dctwrite.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_dctwrite_plan_result.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rsx_samsung_v2_validate.argtypes = [C.c_void_p, C.c_void_p]
        L.rsx_samsung_v2_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_void_p]
        L.rsx_samsung_v1_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_void_p]
        L.rsx_pentax_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p]
        L.rsx_nikon_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p]
        L.rsx_dng_decompress_ljpeg.argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_dng_decompress_uncompressed.argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]
        for name in ("rsx_unpack_plan_create", "rsx_ljpeg_plan_create",
                     "rsx_cr2_plan_create", "rsx_unpack_variant_plan_create",
                     "rsx_nikon_plan_create", "rsx_unpack_f32_plan_create",
                     "rsx_pentax_plan_create", "rsx_samsung_v1_plan_create",
                     "rsx_samsung_v2_plan_create",
                     "rsx_sraw_plan_create", "rsx_hasselblad_plan_create",
                     "rsx_sony_arw1_plan_create", "rsx_phase_one_plan_create",
                     "rsx_sony_arw2_plan_create", "rsx_panasonic_plan_create",
                     "rsx_samsung_v0_plan_create", "rsx_panasonic_v4_plan_create",
                     "rsx_dng_deflate_plan_create", "rsx_nikon_snef_plan_create",
                     "rsx_vc5_plan_create", "rsx_iiq_correct_plan_create",
                     "rsx_dng_post_plan_create", "rsx_bad_pixels_plan_create",
                     "rsx_scale_plan_create", "rsx_dng_jpeg_plan_create",
                     "rsx_fuji_plan_create", "rsx_olympus_plan_create",
                     "rsx_kodak_plan_create", "rsx_crw_plan_create",
                     "rsx_raf_rotate_plan_create", "rsx_sony_srf_plan_create",
                     "rsx_image_hash_plan_create", "rsx_encode_pack_plan_create",
                     "rsx_encode_ljpeg_plan_create", "rsx_fpwrite_pack_plan_create",
                     "rsx_fpwrite_deflate_plan_create", "rsx_dctwrite_plan_create"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p,
                                         C.POINTER(C.c_void_p)]
        L.rsx_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_plan_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsx_plan_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.rsx_plan_kernel_table.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p),
                                            C.POINTER(C.c_double), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int)]
        L.rsx_plan_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_char_p),
                                           C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.rsx_plan_destroy.argtypes = [C.c_void_p]
        L.rsx_probe_stream_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_size_t, C.c_void_p, C.c_int,
                                            C.POINTER(C.c_double)]
        _lib = L
    return _lib


def status_string(st):
    return lib().rsx_status_string(st).decode()


def phase_one_validate(strips, in_bytes, img_view):
    """rsx_phase_one_validate; strips: [(row, offset, bytes)]"""
    arr = abi.phase_one_strips(strips)
    return lib().rsx_phase_one_validate(len(strips), arr, in_bytes, C.byref(img_view))


def sony_arw2_validate(mode, table, img_view, in_bytes):
    """rsx_sony_arw2_validate; mode None passes a NULL desc"""
    if mode is None:
        return lib().rsx_sony_arw2_validate(None, C.byref(img_view), in_bytes)
    d, keep = abi.sony_arw2_desc(mode, table)
    return lib().rsx_sony_arw2_validate(C.byref(d), C.byref(img_view), in_bytes)


def panasonic_validate(version, bps, img_view, in_bytes):
    """rsx_panasonic_validate; version None passes a NULL desc"""
    if version is None:
        return lib().rsx_panasonic_validate(None, C.byref(img_view), in_bytes)
    d = abi.PanasonicDesc(version, bps)
    return lib().rsx_panasonic_validate(C.byref(d), C.byref(img_view), in_bytes)


def panasonic_v4_validate(split, zero_is_bad, img_view, in_bytes):
    """rsx_panasonic_v4_validate; split None passes a NULL desc, img_view None a NULL image"""
    d = None if split is None else C.byref(abi.PanasonicV4Desc(split, int(zero_is_bad)))
    v = None if img_view is None else C.byref(img_view)
    return lib().rsx_panasonic_v4_validate(d, v, in_bytes)


def nikon_snef_validate(inv_wb, table, img_view, in_bytes):
    """rsx_nikon_snef_validate; inv_wb = (r, b), None passes a NULL desc; table None a NULL table"""
    if inv_wb is None:
        return lib().rsx_nikon_snef_validate(None, C.byref(img_view), in_bytes)
    d, keep = abi.nikon_snef_desc(inv_wb[0], inv_wb[1], table)
    return lib().rsx_nikon_snef_validate(C.byref(d), C.byref(img_view), in_bytes)


def vc5_validate(desc, img_view, in_bytes):
    """rsx_vc5_validate; desc: abi.Vc5Desc (abi.vc5_desc), None passes a NULL desc"""
    return lib().rsx_vc5_validate(None if desc is None else C.byref(desc), C.byref(img_view),
                                  in_bytes)


def iiq_correct_validate(corr, img_view):
    """rsx_iiq_correct_validate; corr: abi.IiqCorr (abi.iiq_corr), None passes a NULL list"""
    return lib().rsx_iiq_correct_validate(None if corr is None else C.byref(corr),
                                          C.byref(img_view))


def iiq_defect_positions(payload, dim_x, cap=1 << 16, payload_bytes=None, fn=None):
    """rsx_iiq_defect_positions on the bytes of entry 0x400 (None: a NULL payload).  Returns
    (status, the positions that fit `cap`, the full count).  fn: the same entry point of another
    library (the host build of the core)."""
    a = None if payload is None else np.frombuffer(bytes(payload) + b"\0", dtype=np.uint8)
    n_bytes = (0 if payload is None else len(payload)) if payload_bytes is None else payload_bytes
    buf = (C.c_uint32 * max(1, cap))()
    n = C.c_uint32(0)
    st = (fn or lib().rsx_iiq_defect_positions)(None if a is None else a.ctypes.data, n_bytes, dim_x,
                                                buf, cap, C.byref(n))
    return st, [int(v) for v in buf[:min(cap, n.value)]], n.value


def _bad_out(result, buf, st):
    """the positions a call handed out: None when the list did not fit (or the call failed)"""
    if st != abi.RSX_OK:
        return None
    return [int(v) for v in buf[:result.n_bad]]


def dng_post_validate(desc, img_view, bad_cap=1 << 16):
    """rsx_dng_post_validate; desc: abi.DngPostDesc (abi.dng_post_desc), None passes NULL.
    Returns (status, abi.DngPostResult, host-side positions or None)."""
    r = abi.DngPostResult()
    buf = (C.c_uint32 * max(1, bad_cap))()
    st = lib().rsx_dng_post_validate(None if desc is None else C.byref(desc),
                                     None if img_view is None else C.byref(img_view),
                                     C.byref(r), buf, bad_cap)
    return st, r, _bad_out(r, buf, st)


def dng_lossy_validate(desc, img_view, bad_cap=1 << 16):
    """rsx_dng_lossy_validate; desc: abi.DngLossyDesc (abi.dng_lossy_desc), None passes NULL.
    Returns (status, abi.DngLossyResult, the FixBadPixelsList positions of both lists or None)."""
    r = abi.DngLossyResult()
    buf = (C.c_uint32 * max(1, bad_cap))()
    st = lib().rsx_dng_lossy_validate(None if desc is None else C.byref(desc),
                                      None if img_view is None else C.byref(img_view),
                                      C.byref(r), buf, bad_cap)
    if st != abi.RSX_OK:
        return st, r, None
    return st, r, [int(v) for v in buf[:r.list1.n_bad + r.list2.n_bad]]


def scale_validate(desc, img_view):
    """rsx_scale_validate; desc: abi.ScaleDesc (abi.scale_desc), None passes NULL"""
    return lib().rsx_scale_validate(None if desc is None else C.byref(desc),
                                    None if img_view is None else C.byref(img_view))


def bad_pixels_validate(desc, img_view):
    """rsx_bad_pixels_validate; desc: abi.BadPixelsDesc (abi.bad_pixels_desc), None passes NULL"""
    return lib().rsx_bad_pixels_validate(None if desc is None else C.byref(desc),
                                         None if img_view is None else C.byref(img_view))


def samsung_v0_validate(offsets, in_bytes, img_view, n_offsets=None):
    """rsx_samsung_v0_validate; offsets None passes a NULL table"""
    if offsets is None:
        return lib().rsx_samsung_v0_validate(None, n_offsets or 0, in_bytes, C.byref(img_view))
    arr = abi.samsung_v0_offsets(offsets)
    n = len(offsets) if n_offsets is None else n_offsets
    return lib().rsx_samsung_v0_validate(arr, n, in_bytes, C.byref(img_view))


def fuji_parse(data):
    """rsx_fuji_parse -> (status, abi.FujiDesc)"""
    a = _u8(np.frombuffer(bytes(data) + b"\0", np.uint8))  # (a pointer for no bytes)
    d = abi.FujiDesc()
    return lib().rsx_fuji_parse(a.ctypes.data, len(data), C.byref(d)), d


def fuji_validate(desc, img_view):
    """rsx_fuji_validate; None passes NULL"""
    return lib().rsx_fuji_validate(None if desc is None else C.byref(desc),
                                   None if img_view is None else C.byref(img_view))


def olympus_validate(in_bytes, img_view):
    """rsx_olympus_validate; None passes NULL"""
    return lib().rsx_olympus_validate(in_bytes, None if img_view is None else C.byref(img_view))


def kodak_validate(bps, mode, table, img_view, in_bytes):
    """rsx_kodak_validate; bps None passes a NULL desc, img_view None a NULL image"""
    d, keep = (None, None) if bps is None else abi.kodak_desc(bps, mode, table)
    return lib().rsx_kodak_validate(None if d is None else C.byref(d),
                                    None if img_view is None else C.byref(img_view), in_bytes)


def crw_validate(dec_table, has_lowbits, img_view, in_bytes, low_bytes):
    """rsx_crw_validate; dec_table None passes a NULL desc, img_view None a NULL image"""
    d = None if dec_table is None else abi.crw_desc(dec_table, has_lowbits)
    return lib().rsx_crw_validate(None if d is None else C.byref(d),
                                  None if img_view is None else C.byref(img_view), in_bytes,
                                  low_bytes)


def _ref(x):
    return None if x is None else C.byref(x)


def fuji_rotate_geometry(desc):
    """rsx_raf_rotate_geometry -> (status, out_dim_x, out_dim_y, rotation_pos); desc None passes
    NULL.  The three values are None on any status but RSX_OK."""
    x, y, pos = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    st = lib().rsx_raf_rotate_geometry(_ref(desc), C.byref(x), C.byref(y), C.byref(pos))
    if st != abi.RSX_OK:
        assert (x.value, y.value, pos.value) == (-1, -1, -1), "outputs written on a failure"
        return st, None, None, None
    return st, x.value, y.value, pos.value


def fuji_rotate_validate(desc, src_view, dst_view):
    """rsx_raf_rotate_validate; None passes NULL"""
    return lib().rsx_raf_rotate_validate(_ref(desc), _ref(src_view), _ref(dst_view))


def sony_srf_validate(in_bytes, img_view):
    """rsx_sony_srf_validate; img_view None passes a NULL image"""
    return lib().rsx_sony_srf_validate(in_bytes, _ref(img_view))


def image_hash_validate(img_view, sample_bytes):
    """rsx_image_hash_validate; img_view None passes a NULL image"""
    return lib().rsx_image_hash_validate(_ref(img_view), sample_bytes)


def encode_pack_validate(desc, img_view, out_cap):
    """rsx_encode_pack_validate; None passes NULL"""
    return lib().rsx_encode_pack_validate(_ref(desc), _ref(img_view), out_cap)


def fpwrite_deflate_validate(desc, tile, img_view):
    """rsx_fpwrite_deflate_validate; None passes NULL"""
    return lib().rsx_fpwrite_deflate_validate(_ref(desc), _ref(tile), _ref(img_view))


def fpwrite_deflate_bound(desc, tile, img_view):
    return int(lib().rsx_fpwrite_deflate_bound(_ref(desc), _ref(tile), _ref(img_view)))


def dctwrite_quality_tables(quality):
    """rsx_dctwrite_quality_tables -> (status, luma[64], chroma[64]) in natural order"""
    lu, ch = (C.c_uint16 * 64)(), (C.c_uint16 * 64)()
    st = lib().rsx_dctwrite_quality_tables(quality, lu, ch)
    return st, list(lu), list(ch)


def dctwrite_validate(desc, img_view):
    """rsx_dctwrite_validate; None passes NULL"""
    return lib().rsx_dctwrite_validate(_ref(desc), _ref(img_view))


def dctwrite_bound(desc, img_view):
    return int(lib().rsx_dctwrite_bound(_ref(desc), _ref(img_view)))


def fpwrite_pack_validate(desc, img_view, out_cap):
    """rsx_fpwrite_pack_validate; None passes NULL"""
    return lib().rsx_fpwrite_pack_validate(_ref(desc), _ref(img_view), out_cap)


def encode_ljpeg_validate(desc, img_view):
    """rsx_encode_ljpeg_validate; None passes NULL"""
    return lib().rsx_encode_ljpeg_validate(_ref(desc), _ref(img_view))


def encode_ljpeg_bound(desc, img_view):
    return int(lib().rsx_encode_ljpeg_bound(_ref(desc), _ref(img_view)))


def encode_ljpeg_container(desc, img_view, precision, entropy_bytes=0, cap=1024):
    """rsx_encode_ljpeg_container -> (status, the header's bytes or None)"""
    hdr = np.empty(max(cap, 1), dtype=np.uint8)
    n = C.c_size_t(0)
    st = lib().rsx_encode_ljpeg_container(_ref(desc), _ref(img_view), precision, entropy_bytes,
                                          hdr.ctypes.data, cap, C.byref(n))
    return st, (hdr[:n.value].copy() if st == abi.RSX_OK else None)


def encode_huff_from_histogram(counts, flags=0):
    """rsx_encode_huff_from_histogram: 17 counts -> (status, abi.HuffTable)"""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    assert c.size == abi.ENCODE_CATEGORIES
    t = abi.HuffTable()
    st = lib().rsx_encode_huff_from_histogram(c.ctypes.data, flags, C.byref(t))
    return st, t


def dng_deflate_tile(geom, in_bytes=0, in_ptr=None):
    """geom: (tile_w, tile_h, off_x, off_y, width, height), samples"""
    t = abi.DngDeflateTile()
    t.in_, t.in_bytes = in_ptr, in_bytes
    t.tile_w, t.tile_h, t.off_x, t.off_y, t.width, t.height = geom
    return t


def dng_deflate_validate(bps, predictor, geom, in_bytes, img_view):
    d = abi.DngDeflateDesc(bps, predictor)
    t = dng_deflate_tile(geom, in_bytes)
    return lib().rsx_dng_deflate_validate(C.byref(d), C.byref(t), C.byref(img_view))


def dng_jpeg_validate(stream, off, img_view):
    """rsx_dng_jpeg_validate of one tile; off = (off_x, off_y).  Returns (status, abi.DngJpegInfo)."""
    tiles, keep = abi.dng_jpeg_tiles([stream], [off])
    info = abi.DngJpegInfo()
    st = lib().rsx_dng_jpeg_validate(tiles, C.byref(img_view), C.byref(info))
    return st, info


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a


class Context:
    """rsx_ctx: one per device."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        st = lib().rsx_ctx_create(device, C.byref(self._h))
        if st != abi.RSX_OK:
            raise RsxError(st, "rsx_ctx_create(device=%d): no usable GPU" % device)
        self.device = device

    def last_error(self):
        return lib().rsx_ctx_last_error(self._h).decode(errors="replace")

    def close(self):
        if self._h:
            lib().rsx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def host_calls(self):
        """host-pointer entry points this context has served (rsx_ctx_host_calls)"""
        f = lib().rsx_ctx_host_calls
        f.restype = C.c_uint64
        return int(f(self._h))

    def chunked_calls(self):
        """... of which ran one large stream in chunks (rsx_ctx_chunked_calls)"""
        f = lib().rsx_ctx_chunked_calls
        f.restype = C.c_uint64
        return int(f(self._h))

    # page-locked host memory (rsx.h: optional, ABI 4)
    def host_alloc(self, nbytes):
        """rsx_host_alloc: a page-locked block as a numpy uint8 array (host_free() it)"""
        import numpy as np
        p = C.c_void_p()
        st = lib().rsx_host_alloc(self._h, C.c_size_t(nbytes), C.byref(p))
        if st != 0:
            raise RsxError(st, "rsx_host_alloc(%d)" % nbytes)
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8)
        arr.flags.writeable = True
        return arr

    def host_free(self, arr):
        return lib().rsx_host_free(self._h, C.c_void_p(arr.ctypes.data))

    def host_register(self, arr):
        """rsx_host_register: page-lock an existing numpy array in place (status)"""
        return lib().rsx_host_register(self._h, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes))

    def host_unregister(self, arr):
        return lib().rsx_host_unregister(self._h, C.c_void_p(arr.ctypes.data))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def probe_stream_copy(self, in_ptr, in_bytes, out_ptr, out_bytes, stream=None, reps=20):
        """Average ms of a plain streaming kernel moving in_bytes in / out_bytes out
        (device pointers): the copy ceiling bench.py quotes next to the vendor peak."""
        ms = C.c_double(0)
        st = lib().rsx_probe_stream_copy(self._h, C.c_void_p(in_ptr), in_bytes,
                                         C.c_void_p(out_ptr), out_bytes,
                                         C.c_void_p(stream or 0), reps, C.byref(ms))
        if st != abi.RSX_OK:
            raise RsxError(st, self.last_error())
        return ms.value

    # ---- host-pointer calls (what the patched reference methods call) ------
    def unpack_u16(self, desc, data, img_view):
        a = _u8(data)
        return lib().rsx_unpack_u16(self._h, C.byref(desc), a.ctypes.data, a.size,
                                    C.byref(img_view))

    def unpack_f32(self, desc, data, img_view):
        a = _u8(data)
        return lib().rsx_unpack_f32(self._h, C.byref(desc), a.ctypes.data, a.size,
                                    C.byref(img_view))

    def unpack_variant_u16(self, desc, data, img_view):
        a = _u8(data)
        return lib().rsx_unpack_variant_u16(self._h, C.byref(desc), a.ctypes.data, a.size,
                                            C.byref(img_view))

    def ljpeg_decode(self, desc, data, img_view):
        a = _u8(data)
        consumed = C.c_uint32(0)
        st = lib().rsx_ljpeg_decode(self._h, C.byref(desc), a.ctypes.data, a.size,
                                    C.byref(img_view), C.byref(consumed))
        return st, consumed.value

    def cr2_decode(self, desc, data, img_view):
        a = _u8(data)
        consumed = C.c_uint32(0)
        st = lib().rsx_cr2_decode(self._h, C.byref(desc), a.ctypes.data, a.size,
                                  C.byref(img_view), C.byref(consumed))
        return st, consumed.value

    def sraw_interpolate(self, desc, in_view, out_view):
        return lib().rsx_sraw_interpolate(self._h, C.byref(desc), C.byref(in_view),
                                          C.byref(out_view))

    def nikon_decompress(self, desc, data, img_view):
        a = _u8(data)
        return lib().rsx_nikon_decompress(self._h, C.byref(desc), a.ctypes.data, a.size,
                                          C.byref(img_view))

    def pentax_decompress(self, desc, data, img_view):
        a = _u8(data)
        return lib().rsx_pentax_decompress(self._h, C.byref(desc), a.ctypes.data, a.size,
                                           C.byref(img_view))

    def hasselblad_decompress(self, desc, data, img_view):
        a = _u8(data)
        consumed = C.c_uint32(0)
        st = lib().rsx_hasselblad_decompress(self._h, C.byref(desc), a.ctypes.data, a.size,
                                             C.byref(img_view), C.byref(consumed))
        return st, consumed.value

    def samsung_v1_decompress(self, desc, data, img_view):
        a = _u8(data)
        return lib().rsx_samsung_v1_decompress(self._h, C.byref(desc), a.ctypes.data,
                                               a.size, C.byref(img_view))

    def samsung_v2_decompress(self, desc, data, img_view):
        a = _u8(data)
        return lib().rsx_samsung_v2_decompress(self._h, C.byref(desc), a.ctypes.data,
                                               a.size, C.byref(img_view))

    def sony_arw1_decompress(self, data, img_view):
        a = _u8(data)
        return lib().rsx_sony_arw1_decompress(self._h, a.ctypes.data, a.size,
                                              C.byref(img_view))

    def phase_one_decompress(self, data, strips, img_view):
        """strips: [(row, offset, bytes)] into `data`.  Returns (status, per-row statuses)."""
        a = _u8(data)
        arr = abi.phase_one_strips(strips)
        rows = (C.c_int32 * max(1, img_view.dim_y))()
        st = lib().rsx_phase_one_decompress(self._h, a.ctypes.data, a.size, len(strips), arr,
                                            C.byref(img_view), rows)
        return st, list(rows)[:img_view.dim_y]

    def iiq_correct(self, corr, img_view):
        """corr: abi.IiqCorr; img_view.data a host or a device pointer; in place"""
        return lib().rsx_iiq_correct(self._h, C.byref(corr), C.byref(img_view))

    def phase_one_decompress_corrected(self, data, strips, corr, img_view):
        """phase_one_decompress, then the list `corr` (abi.IiqCorr) on the device, one download.
        Returns (status, per-row statuses)."""
        a = _u8(data)
        arr = abi.phase_one_strips(strips)
        rows = (C.c_int32 * max(1, img_view.dim_y))()
        st = lib().rsx_phase_one_decompress_corrected(self._h, a.ctypes.data, a.size, len(strips),
                                                      arr, C.byref(corr), C.byref(img_view), rows)
        return st, list(rows)[:img_view.dim_y]

    def phase_one_decompress_fixed(self, data, strips, corr, img_view, want_map=True):
        """phase_one_decompress_corrected, then the bad-pixel stage on the positions of the list's
        defects op, one download.  Returns (status, per-row statuses, abi.BadPixelsResult, the map
        as (dim_y, map_pitch) uint8 -- None unless made)."""
        a = _u8(data)
        arr = abi.phase_one_strips(strips)
        rows = (C.c_int32 * max(1, img_view.dim_y))()
        pitch = abi.bad_pixels_map_pitch(img_view.dim_x)
        m = np.full((max(1, img_view.dim_y), pitch), 0xA5, np.uint8)
        r = abi.BadPixelsResult()
        st = lib().rsx_phase_one_decompress_fixed(
            self._h, a.ctypes.data, a.size, len(strips), arr, C.byref(corr), C.byref(img_view), rows,
            m.ctypes.data if want_map else None, pitch if want_map else 0, C.byref(r))
        if want_map and not (st == abi.RSX_OK and r.map_made):
            assert (m == 0xA5).all(), "map_out was written without a map"
        return st, list(rows)[:img_view.dim_y], r, \
            (m if st == abi.RSX_OK and r.map_made and want_map else None)

    def dng_post(self, desc, img_view, bad_cap=1 << 16):
        """desc: abi.DngPostDesc; img_view.data a host or a device pointer; in place.  Returns
        (status, abi.DngPostResult, positions or None)."""
        r = abi.DngPostResult()
        buf = (C.c_uint32 * max(1, bad_cap))()
        st = lib().rsx_dng_post(self._h, C.byref(desc), C.byref(img_view), C.byref(r), buf, bad_cap)
        return st, r, _bad_out(r, buf, st)

    def dng_finish(self, desc, img_view, bad_cap=1 << 16):
        """dng_post, then the bad-pixel stage on the device.  Returns (status, abi.DngPostResult,
        positions or None, the map as (dim_y, map_pitch) uint8 -- untouched 0xA5 unless made)."""
        r = abi.DngPostResult()
        buf = (C.c_uint32 * max(1, bad_cap))()
        m = np.full((img_view.dim_y, abi.bad_pixels_map_pitch(img_view.dim_x)), 0xA5, np.uint8)
        st = lib().rsx_dng_finish(self._h, C.byref(desc), C.byref(img_view), C.byref(r), buf, bad_cap,
                                  m.ctypes.data)
        return st, r, _bad_out(r, buf, st), m

    def _dng_post_call(self, fn, tile_type, descs, datas, desc, img_view, bad_cap, consumed,
                       with_map=False):
        n = len(descs)
        arrs = [_u8(d) for d in datas]
        tiles = (tile_type * n)()
        for i in range(n):
            tiles[i].desc = descs[i]
            tiles[i].in_ = arrs[i].ctypes.data
            tiles[i].in_bytes = arrs[i].size
        # (-1: the call did not write the statuses -- it returned without writing the image)
        st = (C.c_int32 * n)(*([-1] * n))
        r = abi.DngPostResult()
        buf = (C.c_uint32 * max(1, bad_cap))()
        args = [self._h, n, tiles, C.byref(desc), C.byref(img_view), st]
        if consumed:
            args.append(None)
        if with_map:
            m = np.full((img_view.dim_y, abi.bad_pixels_map_pitch(img_view.dim_x)), 0xA5, np.uint8)
            rc = fn(*args, C.byref(r), buf, bad_cap, m.ctypes.data)
            return rc, list(st), r, _bad_out(r, buf, rc), m
        rc = fn(*args, C.byref(r), buf, bad_cap)
        return rc, list(st), r, _bad_out(r, buf, rc)

    def dng_decompress_ljpeg_finish(self, descs, datas, desc, img_view, bad_cap=1 << 16):
        """dng_decompress_ljpeg_post with the bad-pixel stage behind the look-up.  Returns (status,
        tile statuses, result, positions or None, the map -- 0xA5 unless made)."""
        return self._dng_post_call(lib().rsx_dng_decompress_ljpeg_finish, abi.DngLJpegTile, descs,
                                   datas, desc, img_view, bad_cap, True, True)

    def dng_decompress_uncompressed_finish(self, descs, datas, desc, img_view, bad_cap=1 << 16):
        """dng_decompress_uncompressed_post with the bad-pixel stage behind the look-up"""
        return self._dng_post_call(lib().rsx_dng_decompress_uncompressed_finish, abi.DngUnpackTile,
                                   descs, datas, desc, img_view, bad_cap, False, True)

    def dng_decompress_ljpeg_post(self, descs, datas, desc, img_view, bad_cap=1 << 16):
        """dng_decompress_ljpeg, then the list and the look-up of `desc` (abi.DngPostDesc) on the
        device, one download.  Returns (status, tile statuses, result, positions or None)."""
        return self._dng_post_call(lib().rsx_dng_decompress_ljpeg_post, abi.DngLJpegTile, descs,
                                   datas, desc, img_view, bad_cap, True)

    def dng_decompress_uncompressed_post(self, descs, datas, desc, img_view, bad_cap=1 << 16):
        """dng_decompress_uncompressed, then the list and the look-up on the device, one download"""
        return self._dng_post_call(lib().rsx_dng_decompress_uncompressed_post, abi.DngUnpackTile,
                                   descs, datas, desc, img_view, bad_cap, False)

    def bad_pixels_fix(self, desc, img_view):
        """desc: abi.BadPixelsDesc; img_view.data a host or a device pointer; in place.  Returns
        (status, abi.BadPixelsResult)."""
        r = abi.BadPixelsResult()
        st = lib().rsx_bad_pixels_fix(self._h, C.byref(desc), C.byref(img_view), C.byref(r))
        return st, r

    def panasonic_v4_decompress_fixed(self, split, zero_is_bad, data, img_view, want_map=True):
        """panasonic_v4_decompress, then the bad-pixel stage on the device, one download.  Returns
        (status, abi.BadPixelsResult, the map as (dim_y, map_pitch) uint8 -- None unless made)."""
        a = _u8(data)
        d = abi.PanasonicV4Desc(split, int(zero_is_bad))
        pitch = abi.bad_pixels_map_pitch(img_view.dim_x)
        m = np.full((max(1, img_view.dim_y), pitch), 0xA5, np.uint8)
        r = abi.BadPixelsResult()
        st = lib().rsx_panasonic_v4_decompress_fixed(
            self._h, C.byref(d), a.ctypes.data, a.size, C.byref(img_view),
            m.ctypes.data if want_map else None, pitch if want_map else 0, C.byref(r))
        return st, r, (m if st == abi.RSX_OK and r.map_made and want_map else None)

    def sony_arw2_decompress(self, mode, table, data, img_view, rows=True):
        """Returns (status, per-row statuses or None)."""
        a = _u8(data)
        d, keep = abi.sony_arw2_desc(mode, table)
        rs = (C.c_int32 * max(1, img_view.dim_y))() if rows else None
        st = lib().rsx_sony_arw2_decompress(self._h, C.byref(d), a.ctypes.data, a.size,
                                            C.byref(img_view), rs)
        return st, (list(rs)[:img_view.dim_y] if rows else None)

    def panasonic_decompress(self, version, bps, data, img_view):
        a = _u8(data)
        d = abi.PanasonicDesc(version, bps)
        return lib().rsx_panasonic_decompress(self._h, C.byref(d), a.ctypes.data, a.size,
                                              C.byref(img_view))

    def panasonic_v4_decompress(self, split, zero_is_bad, data, img_view, bad_cap=0):
        """Returns (status, the exact count of zero pixels, the sorted list -- None unless the
        status is RSX_OK)."""
        a = _u8(data)
        d = abi.PanasonicV4Desc(split, int(zero_is_bad))
        bad = np.zeros(max(1, bad_cap), np.uint32)
        n = C.c_uint64(0)
        st = lib().rsx_panasonic_v4_decompress(self._h, C.byref(d), a.ctypes.data, a.size,
                                               C.byref(img_view), bad.ctypes.data if bad_cap else None,
                                               bad_cap, C.byref(n))
        return st, n.value, (bad[:n.value].copy() if st == abi.RSX_OK else None)

    def nikon_snef_decompress(self, inv_wb, table, data, img_view):
        """inv_wb = (r, b); table: the dithering TableLookUp's 8192 entries"""
        a = _u8(data)
        d, keep = abi.nikon_snef_desc(inv_wb[0], inv_wb[1], table)
        return lib().rsx_nikon_snef_decompress(self._h, C.byref(d), a.ctypes.data, a.size,
                                               C.byref(img_view))

    def vc5_decompress(self, desc, data, img_view):
        """desc: abi.Vc5Desc with band offsets inside `data` (the tile's bytes)"""
        a = _u8(data)
        return lib().rsx_vc5_decompress(self._h, C.byref(desc), a.ctypes.data, a.size,
                                        C.byref(img_view))

    def samsung_v0_decompress(self, data, offsets, img_view, rows=True):
        """data: the strip; offsets: one per image row.  Returns (status, per-row statuses)."""
        a = _u8(data)
        arr = abi.samsung_v0_offsets(offsets)
        rs = (C.c_int32 * max(1, img_view.dim_y))() if rows else None
        st = lib().rsx_samsung_v0_decompress(self._h, a.ctypes.data, a.size, arr, len(offsets),
                                             C.byref(img_view), rs)
        return st, (list(rs)[:img_view.dim_y] if rows else None)

    def fuji_decompress(self, desc, data, img_view, in_ptr=None, in_bytes=None):
        """desc: abi.FujiDesc with strip offsets inside `data` (host bytes) or inside the device
        buffer at in_ptr (then img_view.data is a device pointer too).  Returns (status, per-strip
        statuses; -1 where the call wrote none)."""
        n = max(0, min(abi.FUJI_MAX_STRIPS, desc.n_strips))
        ss = (C.c_int32 * abi.FUJI_MAX_STRIPS)(*([-1] * abi.FUJI_MAX_STRIPS))
        if in_ptr is None:
            a = _u8(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data)
            in_ptr, in_bytes = a.ctypes.data, a.size
        st = lib().rsx_fuji_decompress(self._h, C.byref(desc), C.c_void_p(in_ptr), in_bytes,
                                       C.byref(img_view), ss)
        return st, list(ss)[:n]

    def olympus_decompress(self, data, img_view, in_ptr=None, in_bytes=None):
        """data: the stream with its 7 leading bytes (host bytes), or the device buffer at in_ptr
        (then img_view.data is a device pointer too).  Returns the status."""
        if in_ptr is None:
            a = _u8(np.frombuffer(bytes(data) + b"\0", np.uint8))  # (a pointer for no bytes)
            in_ptr, in_bytes = a.ctypes.data, len(data)
        return lib().rsx_olympus_decompress(self._h, C.c_void_p(in_ptr), in_bytes,
                                            C.byref(img_view))

    def kodak_decompress(self, bps, mode, table, data, img_view, in_ptr=None, in_bytes=None):
        """data: the stream (host bytes), or the device buffer at in_ptr (then img_view.data is a
        device pointer too).  Returns the status."""
        d, keep = abi.kodak_desc(bps, mode, table)
        if in_ptr is None:
            a = _u8(np.frombuffer(bytes(data) + b"\0", np.uint8))  # (a pointer for no bytes)
            in_ptr, in_bytes = a.ctypes.data, len(data)
        return lib().rsx_kodak_decompress(self._h, C.byref(d), C.c_void_p(in_ptr), in_bytes,
                                          C.byref(img_view))

    def crw_decompress(self, dec_table, data, low, img_view, in_ptr=None, in_bytes=None,
                       low_ptr=None, low_bytes=None):
        """data, low: the scan and the low bits (host bytes; low None: no low bits), or the device
        buffers at in_ptr / low_ptr (then img_view.data is a device pointer too).  Returns the
        status."""
        has_low = low is not None or low_ptr is not None
        d = abi.crw_desc(dec_table, has_low)
        if in_ptr is None:
            a = _u8(np.frombuffer(bytes(data) + b"\0", np.uint8))  # (a pointer for no bytes)
            in_ptr, in_bytes = a.ctypes.data, len(data)
            if has_low:
                b = _u8(np.frombuffer(bytes(low) + b"\0", np.uint8))
                low_ptr, low_bytes = b.ctypes.data, len(low)
        return lib().rsx_crw_decompress(self._h, C.byref(d), C.c_void_p(in_ptr), in_bytes,
                                        C.c_void_p(low_ptr or 0), low_bytes or 0,
                                        C.byref(img_view))

    def fuji_rotate(self, desc, src_view, dst_view):
        """rsx_raf_rotate: both views hold host pointers or both device pointers.  Returns the
        status."""
        return lib().rsx_raf_rotate(self._h, _ref(desc), _ref(src_view), _ref(dst_view))

    def sony_decrypt(self, data, key, in_ptr=None, out_ptr=None, n_words=None):
        """rsx_sony_decrypt.  data: host bytes (a multiple of 4) -> (status, the decrypted bytes);
        or device pointers in_ptr / out_ptr (which may be equal) and n_words -> status."""
        if in_ptr is not None:
            return lib().rsx_sony_decrypt(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), n_words,
                                          key)
        a = _u8(np.frombuffer(bytes(data) + b"\0", np.uint8))  # (a pointer for no bytes)
        out = np.full(len(data) + 1, 0xA5, np.uint8)
        st = lib().rsx_sony_decrypt(self._h, a.ctypes.data, out.ctypes.data, len(data) // 4, key)
        assert out[len(data)] == 0xA5
        return st, out[:len(data)]

    def sony_srf_decompress(self, data, key, img_view, in_ptr=None, in_bytes=None):
        """data: the encrypted image bytes (host), or the device buffer at in_ptr (then
        img_view.data is a device pointer too).  Returns the status."""
        if in_ptr is None:
            a = _u8(np.frombuffer(bytes(data) + b"\0", np.uint8))  # (a pointer for no bytes)
            in_ptr, in_bytes = a.ctypes.data, len(data)
        return lib().rsx_sony_srf_decompress(self._h, C.c_void_p(in_ptr), in_bytes, key,
                                             C.byref(img_view))

    def image_hash(self, img_view, sample_bytes, lines=True):
        """rsx_image_hash: img_view.data is a host or a device pointer.  Returns (status,
        abi.ImageHashResult, the 16 dim_y bytes of the line digests or None without `lines`).
        Both outputs start as 0xA5 bytes, so a call that fails shows that it wrote nothing."""
        r = abi.ImageHashResult()
        C.memset(C.byref(r), 0xA5, C.sizeof(r))
        buf = np.full(16 * max(1, img_view.dim_y), 0xA5, np.uint8) if lines else None
        st = lib().rsx_image_hash(self._h, C.byref(img_view), sample_bytes,
                                  buf.ctypes.data if lines else None, C.byref(r))
        return st, r, (buf.tobytes() if lines else None)

    def dng_decompress_deflate(self, bps, predictor, geoms, datas, img_view):
        """geoms: (tile_w, tile_h, off_x, off_y, width, height) per tile, samples; datas: the
        tiles' zlib streams.  Returns (status, per-tile statuses)."""
        n = len(geoms)
        arrs = [_u8(np.frombuffer(d, np.uint8) if isinstance(d, (bytes, bytearray)) else d)
                for d in datas]
        keep = [a if a.size else np.zeros(1, np.uint8) for a in arrs]  # (a pointer for no bytes)
        tiles = (abi.DngDeflateTile * n)()
        for i in range(n):
            tiles[i] = dng_deflate_tile(geoms[i], arrs[i].size, keep[i].ctypes.data)
        d = abi.DngDeflateDesc(bps, predictor)
        st = (C.c_int32 * n)()
        rc = lib().rsx_dng_decompress_deflate(self._h, C.byref(d), n, tiles, C.byref(img_view), st)
        return rc, list(st)

    def dng_decompress_jpeg(self, streams, offsets, img_view):
        """streams: the tiles' JPEG streams; offsets: (off_x, off_y) per tile, pixels.  Returns
        (status, per-tile statuses)."""
        n = len(streams)
        tiles, keep = abi.dng_jpeg_tiles(streams, offsets)
        st = (C.c_int32 * n)()
        rc = lib().rsx_dng_decompress_jpeg(self._h, n, tiles, C.byref(img_view), st)
        return rc, list(st)

    def dng_lossy_decompress(self, streams, offsets, desc, img_view, bad_cap=1 << 16):
        """The lossy-DNG chain: the JPEG tiles, then list 1 and the look-up, the scaling, list 2 and
        the fix of `desc` (abi.DngLossyDesc) on the device, one download.  Returns (status, tile
        statuses -- -1 where the call did not write them, abi.DngLossyResult, the positions or None
        when they did not fit or no stage ran, the map -- 0xA5 unless made)."""
        n = len(streams)
        tiles, keep = abi.dng_jpeg_tiles(streams, offsets)
        st = (C.c_int32 * n)(*([-1] * n))
        r = abi.DngLossyResult()
        buf = (C.c_uint32 * max(1, bad_cap))()
        m = np.full((img_view.dim_y, abi.bad_pixels_map_pitch(img_view.dim_x)), 0xA5, np.uint8)
        rc = lib().rsx_dng_lossy_decompress(self._h, n, tiles, C.byref(desc), C.byref(img_view), st,
                                            C.byref(r), buf, bad_cap, m.ctypes.data)
        n_bad = r.list1.n_bad + r.list2.n_bad
        bad = [int(v) for v in buf[:n_bad]] if r.stages and n_bad <= bad_cap else None
        del keep
        return rc, list(st), r, bad, m

    def dng_decompress_ljpeg(self, descs, datas, img_view):
        n = len(descs)
        arrs = [_u8(d) for d in datas]
        tiles = (abi.DngLJpegTile * n)()
        for i in range(n):
            tiles[i].desc = descs[i]
            tiles[i].in_ = arrs[i].ctypes.data
            tiles[i].in_bytes = arrs[i].size
        st = (C.c_int32 * n)()
        cons = (C.c_uint32 * n)()
        rc = lib().rsx_dng_decompress_ljpeg(self._h, n, tiles, C.byref(img_view), st,
                                            cons)
        return rc, list(st), list(cons)

    def dng_decompress_uncompressed(self, descs, datas, img_view):
        n = len(descs)
        arrs = [_u8(d) for d in datas]
        tiles = (abi.DngUnpackTile * n)()
        for i in range(n):
            tiles[i].desc = descs[i]
            tiles[i].in_ = arrs[i].ctypes.data
            tiles[i].in_bytes = arrs[i].size
        st = (C.c_int32 * n)()
        rc = lib().rsx_dng_decompress_uncompressed(self._h, n, tiles,
                                                   C.byref(img_view), st)
        return rc, list(st)

    # ---- device-resident plans ---------------------------------------------
    def unpack_plan(self, jobs):
        return Plan(self, "rsx_unpack_plan_create", abi.UnpackJob, jobs)

    def unpack_f32_plan(self, jobs):
        return Plan(self, "rsx_unpack_f32_plan_create", abi.UnpackJob, jobs)

    def unpack_variant_plan(self, jobs):
        return Plan(self, "rsx_unpack_variant_plan_create", abi.UnpackVariantJob, jobs)

    def ljpeg_plan(self, jobs):
        return Plan(self, "rsx_ljpeg_plan_create", abi.LJpegJob, jobs)

    def cr2_plan(self, jobs):
        return Plan(self, "rsx_cr2_plan_create", abi.Cr2Job, jobs)

    def hasselblad_plan(self, jobs):
        return Plan(self, "rsx_hasselblad_plan_create", abi.HasselbladJob, jobs)

    def samsung_v2_plan(self, jobs):
        return Plan(self, "rsx_samsung_v2_plan_create", abi.SamsungV2Job, jobs)

    def samsung_v1_plan(self, jobs):
        return Plan(self, "rsx_samsung_v1_plan_create", abi.SamsungV1Job, jobs)

    def sony_arw1_plan(self, jobs):
        return Plan(self, "rsx_sony_arw1_plan_create", abi.SonyArw1Job, jobs)

    def phase_one_plan(self, jobs):
        """jobs: abi.PhaseOneJob (their strip arrays are copied at plan creation)"""
        return Plan(self, "rsx_phase_one_plan_create", abi.PhaseOneJob, jobs)

    def iiq_correct_plan(self, jobs):
        """jobs: abi.IiqCorrectJob (payloads and curves are copied at plan creation); runs in
        place on the output buffer"""
        return Plan(self, "rsx_iiq_correct_plan_create", abi.IiqCorrectJob, jobs)

    def dng_post_plan(self, jobs):
        """jobs: abi.DngPostJob (lists and tables are parsed and copied at plan creation); runs in
        place on the output buffer"""
        return DngPostPlan(self, "rsx_dng_post_plan_create", abi.DngPostJob, jobs)

    def bad_pixels_plan(self, jobs):
        """jobs: abi.BadPixelsJob (positions in the input buffer; map_in is copied at plan
        creation); runs in place on the output buffer"""
        return BadPixelsPlan(self, "rsx_bad_pixels_plan_create", abi.BadPixelsJob, jobs)

    def scale_black_white(self, desc, img_view):
        """desc: abi.ScaleDesc; img_view describes the uncropped image, .data a host or a device
        pointer; in place.  Returns (status, abi.ScaleResult)."""
        r = abi.ScaleResult()
        st = lib().rsx_scale_black_white(self._h, C.byref(desc), C.byref(img_view), C.byref(r))
        return st, r

    def scale_plan(self, jobs):
        """jobs: abi.ScaleJob (their areas are copied at plan creation); runs in place on the
        output buffer"""
        return ScalePlan(self, "rsx_scale_plan_create", abi.ScaleJob, jobs)

    def sony_arw2_plan(self, jobs):
        """jobs: abi.SonyArw2Job (their tables are copied at plan creation)"""
        return Plan(self, "rsx_sony_arw2_plan_create", abi.SonyArw2Job, jobs)

    def panasonic_plan(self, jobs):
        """jobs: abi.PanasonicJob (versions, depths and geometries may mix)"""
        return Plan(self, "rsx_panasonic_plan_create", abi.PanasonicJob, jobs)

    def panasonic_v4_plan(self, jobs):
        """jobs: abi.PanasonicV4Job (splits, flags and geometries may mix)"""
        return PanasonicV4Plan(self, "rsx_panasonic_v4_plan_create", abi.PanasonicV4Job, jobs)

    def nikon_snef_plan(self, jobs):
        """jobs: abi.NikonSnefJob (their tables are copied at plan creation)"""
        return Plan(self, "rsx_nikon_snef_plan_create", abi.NikonSnefJob, jobs)

    def vc5_plan(self, jobs):
        """jobs: abi.Vc5Job (their code books and log tables are copied at plan creation)"""
        return Vc5Plan(self, "rsx_vc5_plan_create", abi.Vc5Job, jobs)

    def samsung_v0_plan(self, jobs):
        """jobs: abi.SamsungV0Job (their offset arrays are copied at plan creation)"""
        return Plan(self, "rsx_samsung_v0_plan_create", abi.SamsungV0Job, jobs)

    def dng_deflate_plan(self, jobs):
        """jobs: abi.DngDeflateJob, one per tile (depths, predictors and images may mix)"""
        return Plan(self, "rsx_dng_deflate_plan_create", abi.DngDeflateJob, jobs)

    def fuji_plan(self, jobs):
        """jobs: abi.FujiJob, one per frame (types, depths and geometries may mix)"""
        return FujiPlan(self, "rsx_fuji_plan_create", abi.FujiJob, jobs)

    def olympus_plan(self, jobs):
        """jobs: abi.OlympusJob, one per frame (geometries may mix)"""
        return OlympusPlan(self, "rsx_olympus_plan_create", abi.OlympusJob, jobs)

    def kodak_plan(self, jobs):
        """jobs: abi.KodakJob, one per frame (geometries, depths and tables may mix; the tables
        are copied at plan creation)"""
        return Plan(self, "rsx_kodak_plan_create", abi.KodakJob, jobs)

    def crw_plan(self, jobs):
        """jobs: abi.CrwJob, one per frame (geometries and tables may mix)"""
        return CrwPlan(self, "rsx_crw_plan_create", abi.CrwJob, jobs)

    def fuji_rotate_plan(self, jobs):
        """jobs: abi.FujiRotateJob, one per frame (geometries and layouts may mix)"""
        return Plan(self, "rsx_raf_rotate_plan_create", abi.FujiRotateJob, jobs)

    def sony_srf_plan(self, jobs):
        """jobs: abi.SonySrfJob, one per frame (geometries and keys may mix)"""
        return Plan(self, "rsx_sony_srf_plan_create", abi.SonySrfJob, jobs)

    def encode_pack_u16(self, desc, img_view, out_ptr, out_cap):
        """rsx_encode_pack_u16: img_view.data and out_ptr are both host or both device pointers.
        Returns (status, bytes written, stream bytes)."""
        r = abi.EncodePackResult()
        st = lib().rsx_encode_pack_u16(self._h, C.byref(desc), C.byref(img_view), C.c_void_p(out_ptr),
                                       out_cap, C.byref(r))
        return st, int(r.bytes_written), int(r.stream_bytes)

    def encode_ljpeg(self, desc, img_view, flags, out_ptr, out_cap):
        """rsx_encode_ljpeg -> (status, abi.EncodeResult)"""
        r = abi.EncodeResult()
        st = lib().rsx_encode_ljpeg(self._h, C.byref(desc), C.byref(img_view), flags,
                                    C.c_void_p(out_ptr), out_cap, C.byref(r))
        return st, r

    def encode_ljpeg_histogram(self, desc, img_view):
        """rsx_encode_ljpeg_histogram -> (status, counts[4][17] as np.uint64)"""
        counts = np.zeros((4, abi.ENCODE_CATEGORIES), dtype=np.uint64)
        st = lib().rsx_encode_ljpeg_histogram(self._h, C.byref(desc), C.byref(img_view),
                                              counts.ctypes.data)
        return st, counts

    def fpwrite_fit(self, img_view, windows):
        """rsx_fpwrite_fit: windows are (x, y, w, h) in samples; img_view.data is a host or a
        device pointer.  Returns (status, [16 | 24 | 32 per window])."""
        n = len(windows)
        arr = (abi.FpWriteWindow * max(n, 1))(*[abi.FpWriteWindow(*w) for w in windows])
        out = (C.c_int32 * max(n, 1))()
        st = lib().rsx_fpwrite_fit(self._h, C.byref(img_view), n, arr, out)
        return st, list(out)[:n]

    def fpwrite_pack(self, desc, img_view, out_ptr, out_cap):
        """rsx_fpwrite_pack: img_view.data and out_ptr are both host or both device pointers.
        Returns (status, abi.FpWritePackResult)."""
        r = abi.FpWritePackResult()
        st = lib().rsx_fpwrite_pack(self._h, C.byref(desc), C.byref(img_view), C.c_void_p(out_ptr),
                                    out_cap, C.byref(r))
        return st, r

    def fpwrite_deflate(self, desc, tiles, img_view):
        """rsx_fpwrite_deflate: tiles are abi.FpWriteDeflateTile (out pointers on the image's side).
        Returns (status, [abi.FpWriteDeflateResult])."""
        n = len(tiles)
        arr = (abi.FpWriteDeflateTile * n)(*tiles)
        res = (abi.FpWriteDeflateResult * n)()
        st = lib().rsx_fpwrite_deflate(self._h, C.byref(desc), n, arr, C.byref(img_view), res)
        return st, list(res)

    def dctwrite(self, tiles, img_view):
        """rsx_dctwrite: tiles are abi.DctWriteTile (out pointers on the image's side).
        Returns (status, [abi.DctWriteResult])."""
        n = len(tiles)
        arr = (abi.DctWriteTile * n)(*tiles)
        res = (abi.DctWriteResult * n)()
        st = lib().rsx_dctwrite(self._h, n, arr, C.byref(img_view), res)
        return st, list(res)

    def dctwrite_plan(self, jobs):
        """jobs: abi.DctWriteJob, tiles of any geometry; run(images_base, streams_base)"""
        return DctWritePlan(self, "rsx_dctwrite_plan_create", abi.DctWriteJob, jobs)

    def fpwrite_deflate_plan(self, jobs):
        """jobs: abi.FpWriteDeflateJob, the tiles of one or more images; run(images_base,
        streams_base)"""
        return FpWriteDeflatePlan(self, "rsx_fpwrite_deflate_plan_create", abi.FpWriteDeflateJob, jobs)

    def fpwrite_pack_plan(self, jobs):
        """jobs: abi.FpWritePackJob; run(images_base, streams_base)"""
        return FpWritePackPlan(self, "rsx_fpwrite_pack_plan_create", abi.FpWritePackJob, jobs)

    def encode_pack_plan(self, jobs):
        """jobs: abi.EncodePackJob; run(images_base, streams_base)"""
        return Plan(self, "rsx_encode_pack_plan_create", abi.EncodePackJob, jobs)

    def encode_ljpeg_plan(self, jobs):
        """jobs: abi.EncodeLJpegJob (the tiles of a DNG are the jobs of one plan)"""
        return EncodeLJpegPlan(self, "rsx_encode_ljpeg_plan_create", abi.EncodeLJpegJob, jobs)

    def image_hash_plan(self, jobs):
        """jobs: abi.ImageHashJob, one per image (geometries and sample sizes may mix);
        run(images_base, outputs_base)"""
        return Plan(self, "rsx_image_hash_plan_create", abi.ImageHashJob, jobs)

    def dng_jpeg_plan(self, jobs):
        """jobs: abi.DngJpegJob (abi.dng_jpeg_job), one per image"""
        return DngJpegPlan(self, "rsx_dng_jpeg_plan_create", abi.DngJpegJob, jobs)

    def pentax_plan(self, jobs):
        return Plan(self, "rsx_pentax_plan_create", abi.PentaxJob, jobs)

    def sraw_plan(self, jobs):
        return Plan(self, "rsx_sraw_plan_create", abi.SrawJob, jobs)

    def nikon_plan(self, jobs):
        return Plan(self, "rsx_nikon_plan_create", abi.NikonJob, jobs)


class Plan:
    def __init__(self, ctx, create_fn, job_type, jobs):
        self.ctx = ctx
        self.n = len(jobs)
        arr = (job_type * self.n)(*jobs)
        self._h = C.c_void_p()
        st = getattr(lib(), create_fn)(ctx._h, self.n, arr, C.byref(self._h))
        if st != abi.RSX_OK:
            raise RsxError(st, ctx.last_error())

    def run(self, in_ptr, out_ptr, stream=None):
        st = lib().rsx_plan_run(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr),
                                C.c_void_p(stream or 0))
        if st != abi.RSX_OK:
            raise RsxError(st, self.ctx.last_error())

    def results(self):
        st = (C.c_int32 * self.n)()
        cons = (C.c_uint32 * self.n)()
        rc = lib().rsx_plan_results(self._h, st, cons)
        return rc, list(st), list(cons)

    def set_timing(self, on=True):
        lib().rsx_plan_set_timing(self._h, 1 if on else 0)

    def kernel_time(self):
        name = C.c_char_p()
        ms = C.c_double(0)
        n = C.c_int(0)
        st = lib().rsx_plan_kernel_time(self._h, C.byref(name), C.byref(ms),
                                        C.byref(n))
        if st != abi.RSX_OK:
            return None
        return name.value.decode(), ms.value, n.value

    def kernel_table(self, cap=64):
        """[(kernel name, average ms per run)] of the timed runs so far, and the run count
        (LJPEG-family plans; call before kernel_time(), which resets the totals)."""
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        n = C.c_int(0)
        runs = C.c_int(0)
        st = lib().rsx_plan_kernel_table(self._h, cap, names, ms, C.byref(n), C.byref(runs))
        if st != abi.RSX_OK:
            return None
        return [(names[i].decode(), ms[i]) for i in range(min(cap, n.value))], runs.value

    def close(self):
        if self._h:
            lib().rsx_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DngPostPlan(Plan):
    def result(self, job):
        r = abi.DngPostResult()
        st = lib().rsx_dng_post_plan_result(self._h, job, C.byref(r))
        return st, r

    def bad_pixels(self, job, cap):
        """(status, exact count, positions or None) of job `job` behind results()"""
        buf = (C.c_uint32 * max(1, cap))()
        n = C.c_uint64(0)
        st = lib().rsx_dng_post_plan_bad_pixels(self._h, job, buf if cap else None, cap, C.byref(n))
        return st, n.value, ([int(v) for v in buf[:n.value]] if st == abi.RSX_OK else None)


class BadPixelsPlan(Plan):
    def result(self, job):
        """after results(): (status, abi.BadPixelsResult) of job `job`"""
        r = abi.BadPixelsResult()
        st = lib().rsx_bad_pixels_plan_result(self._h, job, C.byref(r))
        return st, r


class FpWriteDeflatePlan(Plan):
    def result(self, job):
        """after results(): (status, abi.FpWriteDeflateResult) of job `job`"""
        r = abi.FpWriteDeflateResult()
        st = lib().rsx_fpwrite_deflate_plan_result(self._h, job, C.byref(r))
        return st, r


class DctWritePlan(Plan):
    def result(self, job):
        """after results(): (status, abi.DctWriteResult) of job `job`"""
        r = abi.DctWriteResult()
        st = lib().rsx_dctwrite_plan_result(self._h, job, C.byref(r))
        return st, r


class FpWritePackPlan(Plan):
    def result(self, job):
        """after results(): (status, abi.FpWritePackResult) of job `job`"""
        r = abi.FpWritePackResult()
        st = lib().rsx_fpwrite_pack_plan_result(self._h, job, C.byref(r))
        return st, r


class EncodeLJpegPlan(Plan):
    def result(self, job):
        """after results(): (status, abi.EncodeResult) of job `job`"""
        r = abi.EncodeResult()
        st = lib().rsx_encode_ljpeg_plan_result(self._h, job, C.byref(r))
        return st, r


class ScalePlan(Plan):
    def result(self, job):
        """after results(): (status, abi.ScaleResult) of job `job`"""
        r = abi.ScaleResult()
        st = lib().rsx_scale_plan_result(self._h, job, C.byref(r))
        return st, r


class DngJpegPlan(Plan):
    def tile_status(self, job, n_tiles):
        """after results(): (status, the statuses of the job's tiles)"""
        st = (C.c_int32 * max(1, n_tiles))()
        rc = lib().rsx_dng_jpeg_plan_tile_status(self._h, job, st)
        return rc, list(st)[:n_tiles]


class FujiPlan(Plan):
    def strip_status(self, job, n_strips):
        """after results(): (status, the statuses of the job's strips)"""
        st = (C.c_int32 * max(1, n_strips))()
        rc = lib().rsx_fuji_plan_strip_status(self._h, job, st)
        return rc, list(st)[:n_strips]


class OlympusPlan(Plan):
    def job_status(self, job):
        """after results(): (status of the getter, the job's status)"""
        st = C.c_int32(-1)
        rc = lib().rsx_olympus_plan_job_status(self._h, job, C.byref(st))
        return rc, st.value


class PanasonicV4Plan(Plan):
    def bad_pixels(self, job, cap):
        """after results(): (status, the exact count, the job's sorted list -- None unless RSX_OK)"""
        bad = np.zeros(max(1, cap), np.uint32)
        n = C.c_uint64(0)
        st = lib().rsx_panasonic_v4_plan_bad_pixels(self._h, job, bad.ctypes.data if cap else None,
                                                    cap, C.byref(n))
        return st, n.value, (bad[:n.value].copy() if st == abi.RSX_OK else None)


class CrwPlan(Plan):
    def stats(self, job):
        """after results(): (windows, inner rounds, outer rounds used, settling work) of job
        `job` of the last run"""
        v = (C.c_uint32 * 4)()
        rc = lib().rsx_crw_plan_stats(self._h, job, v)
        if rc != abi.RSX_OK:
            raise RsxError(rc, "rsx_crw_plan_stats")
        return tuple(int(x) for x in v)


class Vc5Plan(Plan):
    def bands(self, job):
        """after results(): (band status, windows, parse rounds), each a (4, 10) array
        [channel][subband]"""
        st = np.zeros((4, 10), np.int32)
        win = np.zeros((4, 10), np.uint32)
        rnd = np.zeros((4, 10), np.uint32)
        rc = lib().rsx_vc5_plan_bands(self._h, job, st.ctypes.data, win.ctypes.data, rnd.ctypes.data)
        if rc != abi.RSX_OK:
            raise RsxError(rc, "rsx_vc5_plan_bands")
        return st, win, rnd
