"""ctypes binding of include/miphy.h.  No torch types cross the C ABI: tensors are passed as raw device pointers."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIPHY_LIBRARY: another build of the same library (tools/ab_bench.py compares kernel variants this way)
lib_path = os.environ.get("MIPHY_LIBRARY") or os.path.join(os.path.dirname(_HERE), "libmiphy.so")

CRC24A, CRC24B, CRC24C, CRC16, CRC11 = range(5)
CRC_NONE = 255


class LibraryNotBuilt(RuntimeError):
    pass


_lib = None


def lib():
    """Loads libmiphy.so (torch must already be imported so that its HIP runtime is the one in the process)."""
    global _lib
    if _lib is None:
        if not os.path.exists(lib_path):
            raise LibraryNotBuilt("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
                                  "srsran_project_23.5_amd`. There is no CPU fallback." % lib_path)
        import torch  # noqa: F401  (loads libamdhip64 first; the C ABI itself has no torch dependency)
        l = C.CDLL(lib_path)
        l.miphy_last_error.restype = C.c_char_p
        l.miphy_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        l.miphy_destroy.argtypes = [C.c_void_p]
        l.miphy_ldpc_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("miphy_ldpc_rate_match_batch", "miphy_ldpc_encode_batch"):
            getattr(l, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_ldpc_rate_dematch_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]
        l.miphy_dft_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("miphy_ofdm_demodulate_slots", "miphy_ofdm_modulate_slots"):
            getattr(l, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_ofdm_slot_size.argtypes = [C.c_void_p, C.c_uint32]
        l.miphy_ofdm_slot_size.restype = C.c_uint32
        l.miphy_dmrs_pusch_estimate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]
        l.miphy_port_channel_estimate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p]
        l.miphy_polar_code_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_polar_encode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_polar_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pdcch_encode_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pusch_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
        l.miphy_pdsch_encode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pusch_decode_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        l.miphy_pusch_decode_plan_run.argtypes = [C.c_void_p] * 8
        l.miphy_pusch_decode_plan_destroy.argtypes = [C.c_void_p]
        l.miphy_pusch_decode_plan_destroy.restype = None
        l.miphy_pusch_decode_plan_enable_timing.argtypes = [C.c_void_p, C.c_uint32]
        l.miphy_pusch_decode_plan_read_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pusch_decode_plan_info.argtypes = [C.c_void_p, C.c_void_p]
        l.miphy_pusch_decode_plan_nof_launches.argtypes = [C.c_void_p]
        l.miphy_pusch_decode_plan_nof_launches.restype = C.c_uint32
        l.miphy_sch_segmentation_info.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        l.miphy_pdsch_process_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        l.miphy_pdsch_process_plan_run.argtypes = [C.c_void_p] * 4
        l.miphy_pdsch_process_plan_destroy.argtypes = [C.c_void_p]
        l.miphy_pdsch_process_plan_destroy.restype = None
        l.miphy_ldpc_decode_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        l.miphy_ldpc_decode_plan_run.argtypes = [C.c_void_p] * 5
        l.miphy_ldpc_decode_plan_nof_launches.argtypes = [C.c_void_p]
        l.miphy_ldpc_decode_plan_nof_launches.restype = C.c_uint32
        l.miphy_ldpc_decode_plan_destroy.argtypes = [C.c_void_p]
        l.miphy_ldpc_decode_plan_destroy.restype = None
        l.miphy_debug_ldpc_kernels_used.argtypes = [C.c_int]
        l.miphy_debug_ldpc_kernels_used.restype = C.c_uint32
        if hasattr(l, "miphy_ldpc_address_table"):  # (an older build named by MIPHY_LIBRARY for an A-B has neither)
            l.miphy_ldpc_address_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
            l.miphy_debug_ldpc_address_table_launches.argtypes = [C.c_int]
            l.miphy_debug_ldpc_address_table_launches.restype = C.c_uint32
        l.miphy_polar_decode_list_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pbch_encode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_crc_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pusch_demodulate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        l.miphy_pdsch_modulate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_dmrs_pdsch_map_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_pdsch_mod_nof_re.argtypes = [C.c_void_p]
        l.miphy_pdsch_mod_nof_re.restype = C.c_uint32
        l.miphy_pusch_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 8
        l.miphy_pusch_demod_nof_llr.argtypes = [C.c_void_p]
        l.miphy_pdsch_pdu_nof_re.argtypes = [C.c_void_p]
        l.miphy_pdsch_pdu_nof_re.restype = C.c_uint32
        l.miphy_pdsch_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pdsch_modulate_layers_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pdsch_mod_layers_nof_re.argtypes = [C.c_void_p]
        l.miphy_pdsch_mod_layers_nof_re.restype = C.c_uint32
        l.miphy_pdsch_layers_pdu_nof_re.argtypes = [C.c_void_p]
        l.miphy_pdsch_layers_pdu_nof_re.restype = C.c_uint32
        l.miphy_pdsch_process_layers_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_vrb_to_prb_list.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_pdsch_modulate_mapped_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_pdsch_process_mapped_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_pdsch_modulate_codewords_batch"):  # (an older build named by MIPHY_LIBRARY for an A-B has none of them)
            l.miphy_pdsch_modulate_codewords_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            l.miphy_pdsch_process_codewords_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            for f in (l.miphy_pdsch_mod_codewords_nof_re, l.miphy_pdsch_codewords_pdu_nof_re):
                f.argtypes = [C.c_void_p]
                f.restype = C.c_uint32
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_channel_precode_batch"):  # (an older build named by MIPHY_LIBRARY for an A-B has none of them)
            l.miphy_channel_precode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            l.miphy_pdsch_modulate_precoded_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                              C.c_void_p, C.c_void_p]
            l.miphy_dmrs_pdsch_map_precoded_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            l.miphy_pdsch_process_precoded_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                             C.c_void_p, C.c_void_p]
        l.miphy_ofh_iq_decompress_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        l.miphy_ofh_iq_compress_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        l.miphy_pdcch_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_ssb_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_csi_rs_map_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_harq_pool_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        l.miphy_harq_pool_destroy.argtypes = [C.c_void_p]
        l.miphy_harq_pool_destroy.restype = None
        l.miphy_harq_pool_reserve.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
        for name in ("miphy_harq_pool_lock", "miphy_harq_pool_unlock", "miphy_harq_pool_release"):
            getattr(l, name).argtypes = [C.c_void_p, C.c_int32]
        l.miphy_harq_pool_run_slot.argtypes = [C.c_void_p, C.c_uint32]
        l.miphy_harq_pool_info.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        l.miphy_harq_pool_free_codeblocks.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        l.miphy_harq_pool_arrays.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
        l.miphy_pusch_demod_nof_llr.restype = C.c_uint32
        l.miphy_pusch_process_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 10
        l.miphy_pusch_demodulate_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 7
        l.miphy_ulsch_demux_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_ulsch_placeholders.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        l.miphy_ulsch_demultiplex_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        l.miphy_channel_equalize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_pusch_demodulate_layers_batch"):  # (an older build named by MIPHY_LIBRARY for an A-B has none of them)
            l.miphy_channel_equalize_layers_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
            l.miphy_pusch_demodulate_layers_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
            l.miphy_pusch_demod_layers_nof_llr.argtypes = [C.c_void_p]
            l.miphy_pusch_demod_layers_nof_llr.restype = C.c_uint32
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_pusch_process_layers_batch"):  # (likewise)
            l.miphy_dmrs_pusch_estimate_layers_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 4
            l.miphy_pusch_process_layers_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 8
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_pusch_process_layers_batch_ex"):  # (likewise)
            l.miphy_pusch_demodulate_layers_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 7
            l.miphy_pusch_process_layers_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 10
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_pusch_demodulate_tp_batch"):  # (likewise)
            l.miphy_transform_deprecode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
            l.miphy_pusch_demodulate_tp_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
            l.miphy_pusch_demodulate_tp_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 7
            l.miphy_low_papr_sequence.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
            l.miphy_dmrs_pusch_tp_pilots_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
            l.miphy_dmrs_pusch_estimate_tp_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 4
            l.miphy_pusch_process_tp_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 8
            l.miphy_pusch_process_tp_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 10
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_channel_equalize_mmse_batch"):  # (likewise)
            l.miphy_pusch_noise_covariance_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 3
            l.miphy_pusch_noise_covariance_nof_prg.argtypes = [C.c_void_p]
            l.miphy_pusch_noise_covariance_nof_prg.restype = C.c_uint32
            l.miphy_channel_equalize_mmse_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 6
            l.miphy_pusch_demodulate_layers_mmse_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 6
            l.miphy_pusch_demodulate_layers_mmse_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 8
            l.miphy_pusch_process_layers_mmse_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 10
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_dmrs_pusch_estimate_cfo_batch"):  # (likewise)
            l.miphy_dmrs_pusch_estimate_cfo_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
            l.miphy_pusch_process_layers_cfo_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 11
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_dmrs_pusch_estimate_tv_batch"):  # (likewise)
            l.miphy_dmrs_pusch_estimate_tv_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 6
            l.miphy_pusch_process_layers_tv_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 10 + [C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_polar_block_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("miphy_ofdm_demodulate_symbols", "miphy_ofdm_modulate_symbols"):
            getattr(l, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.miphy_ofdm_symbol_size.argtypes = [C.c_void_p, C.c_uint32]
        l.miphy_ofdm_symbol_size.restype = C.c_uint32
        l.miphy_uci_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 4
        l.miphy_pusch_uci_field_jobs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
        l.miphy_uci_polar_info.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        l.miphy_uci_polar_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
        l.miphy_pusch_uci_jobs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        l.miphy_debug_set_uci_polar_piece_bytes.argtypes = [C.c_size_t]
        l.miphy_debug_set_uci_polar_piece_bytes.restype = None
        l.miphy_debug_uci_polar_pieces.restype = C.c_uint
        l.miphy_uci_polar_decode_list_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        l.miphy_debug_uci_polar_list_segments.argtypes = [C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        l.miphy_debug_uci_polar_list_segments.restype = None
        l.miphy_pucch_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
        l.miphy_pucch_process_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
        l.miphy_pucch_f34_info.argtypes = [C.c_void_p, C.c_void_p]
        l.miphy_pucch_process_f34_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6
        l.miphy_pucch_f0_info.argtypes = [C.c_void_p, C.c_void_p]
        l.miphy_pucch_process_f0_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 5
        l.miphy_srs_info.argtypes = [C.c_void_p, C.c_void_p]
        l.miphy_srs_pilots_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 2
        l.miphy_srs_estimate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 4
        if not os.environ.get("MIPHY_LIBRARY") or hasattr(l, "miphy_precoding_weights_batch"):  # (an older build named by MIPHY_LIBRARY for an A-B has neither)
            l.miphy_precoding_weights_info.argtypes = [C.c_void_p, C.c_void_p]
            l.miphy_precoding_weights_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_prach_detect_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 4
        l.miphy_prach_generate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 2
        l.miphy_prach_demod_info.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
        l.miphy_prach_demodulate_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
        _lib = l
    return _lib


# Mirrors miphy_ldpc_dec_desc.
LdpcDecDesc = np.dtype([("bg", np.uint8), ("crc_poly", np.uint8), ("Z", np.uint16), ("max_iter", np.uint16),
                        ("nof_filler_bits", np.uint16), ("in_len", np.uint32), ("flags", np.uint32),
                        ("llr_offset", np.uint64), ("out_offset", np.uint64)], align=True)
assert LdpcDecDesc.itemsize == 32
# Mirrors miphy_ldpc_rdm_desc.
LdpcRdmDesc = np.dtype([("bg", np.uint8), ("rv", np.uint8), ("mod", np.uint8), ("new_data", np.uint8), ("Z", np.uint16),
                        ("nof_filler_bits", np.uint16), ("Nref", np.uint32), ("E", np.uint32), ("in_offset", np.uint64),
                        ("out_offset", np.uint64)], align=True)
assert LdpcRdmDesc.itemsize == 32
# Mirrors miphy_ldpc_enc_desc.
LdpcEncDesc = np.dtype([("bg", np.uint8), ("reserved0", np.uint8), ("Z", np.uint16), ("out_len", np.uint32),
                        ("in_offset", np.uint64), ("out_offset", np.uint64)], align=True)
assert LdpcEncDesc.itemsize == 24
# Mirrors miphy_ofdm_job.
OfdmJob = np.dtype([("samples_offset", np.uint64), ("grid_offset", np.uint64), ("slot_index", np.uint32), ("grid_empty", np.uint32)],
                   align=True)
assert OfdmJob.itemsize == 24


class OfdmConfig(C.Structure):
    """Mirrors miphy_ofdm_config (= srsran::ofdm_demodulator_configuration / ofdm_modulator_configuration)."""
    _fields_ = [("numerology", C.c_uint32), ("bw_rb", C.c_uint32), ("dft_size", C.c_uint32),
                ("nof_samples_window_offset", C.c_uint32), ("scale", C.c_float), ("reserved", C.c_float),
                ("center_freq_hz", C.c_double)]

    def slot_size(self, slot_index):
        return int(lib().miphy_ofdm_slot_size(C.byref(self), slot_index))

    def symbol_size(self, symbol_index):
        """Samples (cyclic prefix included) of OFDM symbol `symbol_index` of the subframe."""
        return int(lib().miphy_ofdm_symbol_size(C.byref(self), symbol_index))


def ofdm_symbol_size(cfg, symbol_index):
    return cfg.symbol_size(symbol_index)


# Mirrors miphy_pusch_chest_job.
PuschChestJob = np.dtype([("numerology", np.uint32), ("slot_in_frame", np.uint32), ("scrambling_id", np.uint32), ("scaling", np.float32),
                          ("n_scid", np.uint8), ("nof_tx_layers", np.uint8), ("nof_rx_ports", np.uint8), ("first_symbol", np.uint8),
                          ("nof_symbols", np.uint8), ("rx_ports", np.uint8, 4), ("ce_compact", np.uint8), ("reserved", np.uint8, 2), ("symbols_mask", np.uint16),
                          ("grid_nof_prb", np.uint16), ("rb_mask", np.uint64, 5), ("grid_offset", np.uint64), ("ce_offset", np.uint64),
                          ("scalars_offset", np.uint64), ("rb_mask2", np.uint64, 5), ("pilots_offset", np.uint64), ("hop_symbol", np.uint8),
                          ("re_odd_mask", np.uint8), ("reserved2", np.uint8, 6)], align=True)
assert PuschChestJob.itemsize == 152, PuschChestJob.itemsize
assert PuschChestJob.fields["rb_mask"][1] == 32 and PuschChestJob.fields["symbols_mask"][1] == 28


# Mirrors miphy_pusch_ncov_job: the noise-plus-interference covariance of an allocation, one P x P matrix per PRG.
PuschNcovJob = np.dtype([("base", PuschChestJob), ("cov_offset", np.uint64), ("loading", np.float32), ("prg_size", np.uint16), ("reserved", np.uint8, 2)],
                        align=True)
assert PuschNcovJob.itemsize == 168 and PuschNcovJob.fields["cov_offset"][1] == 152, PuschNcovJob.itemsize


# Mirrors miphy_pusch_chest_cfo_job: the layered estimator with the carrier frequency offset estimated and compensated; {cfo_hz, rho} at cfo_offset.
PuschChestCfoJob = np.dtype([("base", PuschChestJob), ("cfo_offset", np.uint64)], align=True)
assert PuschChestCfoJob.itemsize == 160 and PuschChestCfoJob.fields["cfo_offset"][1] == 152, PuschChestCfoJob.itemsize


# Mirrors miphy_pusch_chest_tv_job: the CFO estimator for a channel that changes within the slot; the variation of (port, layer) at var_offset +
# port * nof_tx_layers + layer; time_mode TIME_INTERPOLATE or TIME_LINE.
TIME_INTERPOLATE, TIME_LINE = 1, 2
PuschChestTvJob = np.dtype([("base", PuschChestCfoJob), ("var_offset", np.uint64), ("time_mode", np.uint8), ("reserved", np.uint8, 7)], align=True)
assert PuschChestTvJob.itemsize == 176 and PuschChestTvJob.fields["var_offset"][1] == 160 and PuschChestTvJob.fields["time_mode"][1] == 168, PuschChestTvJob.itemsize


def pusch_noise_covariance_nof_prg(job):
    """Matrices one PuschNcovJob record writes (host computation in the library); 0 for an invalid one."""
    a = np.ascontiguousarray(np.asarray(job, dtype=PuschNcovJob).reshape(1))
    return int(lib().miphy_pusch_noise_covariance_nof_prg(a.ctypes.data_as(C.c_void_p)))


# Mirrors miphy_pusch_demod_job.
PuschDemodJob = np.dtype([("rnti", np.uint32), ("n_id", np.uint32), ("mod", np.uint8), ("nof_rx_ports", np.uint8), ("start_symbol", np.uint8),
                          ("nof_symbols", np.uint8), ("dmrs_type", np.uint8), ("nof_cdm_groups_without_data", np.uint8),
                          ("ce_nof_symbols", np.uint8), ("ce_compact", np.uint8), ("rx_ports", np.uint8, 4), ("dmrs_symbols_mask", np.uint16),
                          ("grid_nof_prb", np.uint16), ("nof_llr", np.uint32), ("rb_mask", np.uint64, 5), ("grid_offset", np.uint64),
                          ("ce_offset", np.uint64), ("scalars_offset", np.uint64), ("llr_offset", np.uint64), ("placeholders_offset", np.uint32),
                          ("nof_placeholders", np.uint32), ("evm_offset", np.uint64)], align=True)
assert PuschDemodJob.itemsize == 120 and PuschDemodJob.fields["rb_mask"][1] == 32, PuschDemodJob.itemsize


def pusch_demod_nof_llr(job):
    """Codeword length (data REs x bits per symbol) of one PuschDemodJob record (host computation in the library)."""
    a = np.ascontiguousarray(np.asarray(job, dtype=PuschDemodJob).reshape(1))
    return int(lib().miphy_pusch_demod_nof_llr(a.ctypes.data_as(C.c_void_p)))


# Mirrors miphy_pusch_demod_layers_job: one codeword on 1..4 transmit layers.
PuschDemodLayersJob = np.dtype([("base", PuschDemodJob), ("nof_tx_layers", np.uint8), ("reserved", np.uint8, 7)], align=True)
assert PuschDemodLayersJob.itemsize == 128 and PuschDemodLayersJob.fields["nof_tx_layers"][1] == 120, PuschDemodLayersJob.itemsize


def pusch_demod_layers_nof_llr(job):
    """Codeword length (data REs x layers x bits per symbol) of one PuschDemodLayersJob record; 0 for an invalid one."""
    a = np.ascontiguousarray(np.asarray(job, dtype=PuschDemodLayersJob).reshape(1))
    return int(lib().miphy_pusch_demod_layers_nof_llr(a.ctypes.data_as(C.c_void_p)))


# Mirrors miphy_pusch_demod_mmse_job: a layered demodulator job and its covariance matrices.
PuschDemodMmseJob = np.dtype([("base", PuschDemodLayersJob), ("cov_offset", np.uint64), ("prg_size", np.uint16), ("reserved", np.uint8, 6)], align=True)
assert PuschDemodMmseJob.itemsize == 144 and PuschDemodMmseJob.fields["cov_offset"][1] == 128, PuschDemodMmseJob.itemsize


# Transform precoding (DFT-s-OFDM). Mirrors miphy_transform_deprecode_job and miphy_pusch_chest_tp_job.
TransformDeprecodeJob = np.dtype([("M", np.uint32), ("nof_symbols", np.uint32), ("eq_symbols_offset", np.uint64), ("eq_noise_vars_offset", np.uint64),
                                  ("out_symbols_offset", np.uint64), ("out_noise_var_offset", np.uint64)], align=True)
assert TransformDeprecodeJob.itemsize == 40
PuschChestTpJob = np.dtype([("base", PuschChestJob), ("hopping", np.uint8), ("reserved", np.uint8, 7)], align=True)
assert PuschChestTpJob.itemsize == 160 and PuschChestTpJob.fields["hopping"][1] == 152, PuschChestTpJob.itemsize


def low_papr_sequence(u, v, length):
    """r_{u,v}(n), alpha = 0, of TS 38.211 5.2.2 as complex64 (host computation in the library): length 12, 30 or 6 N >= 36."""
    out = np.zeros(int(length), dtype=np.complex64)
    check(lib().miphy_low_papr_sequence(int(u), int(v), int(length), out.ctypes.data_as(C.c_void_p)))
    return out


# Mirrors miphy_re_pattern / miphy_pdsch_mod_job / miphy_dmrs_pdsch_job.
RePattern = np.dtype([("prb_mask", np.uint64, 5), ("re_mask", np.uint16), ("symbols", np.uint16), ("pad", np.uint32)], align=True)
PdschModJob = np.dtype([("rnti", np.uint32), ("n_id", np.uint32), ("scaling", np.float32), ("mod", np.uint8), ("port", np.uint8),
                        ("start_symbol", np.uint8), ("nof_symbols", np.uint8), ("dmrs_type", np.uint8), ("nof_cdm_groups_without_data", np.uint8),
                        ("nof_reserved", np.uint8), ("reserved0", np.uint8), ("dmrs_symbols_mask", np.uint16), ("grid_nof_prb", np.uint16),
                        ("bwp_start_rb", np.uint16), ("bwp_size_rb", np.uint16), ("nof_bits", np.uint32), ("rb_mask", np.uint64, 5),
                        ("reserved", RePattern, 4), ("cw_offset", np.uint64), ("grid_offset", np.uint64)], align=True)
assert RePattern.itemsize == 48 and PdschModJob.itemsize == 280 and PdschModJob.fields["rb_mask"][1] == 32, PdschModJob.itemsize
DmrsPdschJob = np.dtype([("slot_in_frame", np.uint32), ("reference_point_k_rb", np.uint32), ("scrambling_id", np.uint32), ("amplitude", np.float32),
                         ("dmrs_type", np.uint8), ("n_scid", np.uint8), ("nof_ports", np.uint8), ("reserved0", np.uint8), ("ports", np.uint8, 12),
                         ("symbols_mask", np.uint16), ("grid_nof_prb", np.uint16), ("pad", np.uint32), ("rb_mask", np.uint64, 5),
                         ("grid_offset", np.uint64)], align=True)
assert DmrsPdschJob.itemsize == 88 and DmrsPdschJob.fields["rb_mask"][1] == 40, DmrsPdschJob.itemsize


def pdsch_mod_nof_re(job):
    """Data REs of one PdschModJob record (host computation in the library)."""
    a = np.ascontiguousarray(np.asarray(job, dtype=PdschModJob).reshape(1))
    return int(lib().miphy_pdsch_mod_nof_re(a.ctypes.data_as(C.c_void_p)))


# Mirrors miphy_pdsch_mod_layers_job: one codeword on 1..4 layers, layer ly on grid port ports[ly].
PdschModLayersJob = np.dtype([("base", PdschModJob), ("nof_layers", np.uint8), ("ports", np.uint8, 4), ("pad", np.uint8, 3)], align=True)
assert PdschModLayersJob.itemsize == 288 and PdschModLayersJob.fields["nof_layers"][1] == 280 and PdschModLayersJob.fields["ports"][1] == 281


def pdsch_mod_layers_nof_re(job):
    """Data REs per layer of one PdschModLayersJob record (host computation in the library); 0 on an invalid job."""
    a = np.ascontiguousarray(np.asarray(job, dtype=PdschModLayersJob).reshape(1))
    return int(lib().miphy_pdsch_mod_layers_nof_re(a.ctypes.data_as(C.c_void_p)))


# Mirrors miphy_ofh_iq_job.
OfhIqJob = np.dtype([("payload_offset", np.uint64), ("grid_offset", np.uint64), ("nof_prb", np.uint32), ("data_width", np.uint16),
                     ("compression", np.uint16)], align=True)
OFH_COMPRESSION_NONE, OFH_COMPRESSION_BFP = 0, 1  # srsran::ofh::compression_type
assert OfhIqJob.itemsize == 24

# Mirrors miphy_pdsch_pdu.
PdschPdu = np.dtype([("slot_in_frame", np.uint32), ("rnti", np.uint32), ("n_id", np.uint32), ("dmrs_scrambling_id", np.uint32),
                     ("tbs_lbrm_bytes", np.uint32), ("tb_bytes", np.uint32), ("ratio_pdsch_dmrs_to_sss_dB", np.float32),
                     ("ratio_pdsch_data_to_sss_dB", np.float32), ("bg", np.uint8), ("rv", np.uint8), ("mod", np.uint8), ("port", np.uint8),
                     ("start_symbol", np.uint8), ("nof_symbols", np.uint8), ("nof_cdm_groups_without_data", np.uint8), ("n_scid", np.uint8),
                     ("ref_point_prb0", np.uint8), ("nof_reserved", np.uint8), ("dmrs_symbols_mask", np.uint16), ("grid_nof_prb", np.uint16),
                     ("bwp_start_rb", np.uint16), ("bwp_size_rb", np.uint16), ("pad", np.uint16), ("rb_mask", np.uint64, 5),
                     ("reserved", RePattern, 4), ("tb_offset", np.uint64), ("grid_offset", np.uint64)], align=True)
assert PdschPdu.itemsize == 304 and PdschPdu.fields["rb_mask"][1] == 56, PdschPdu.itemsize


def pdsch_pdu_nof_re(pdu):
    """Data REs of one PdschPdu record (pdsch_processor_impl::compute_nof_data_re; host computation in the library)."""
    a = np.ascontiguousarray(np.asarray(pdu, dtype=PdschPdu).reshape(1))
    return int(lib().miphy_pdsch_pdu_nof_re(a.ctypes.data_as(C.c_void_p)))


# Mirrors miphy_pdsch_layers_pdu.
PdschLayersPdu = np.dtype([("base", PdschPdu), ("nof_layers", np.uint8), ("ports", np.uint8, 4), ("pad", np.uint8, 3)], align=True)
assert PdschLayersPdu.itemsize == 312 and PdschLayersPdu.fields["nof_layers"][1] == 304 and PdschLayersPdu.fields["ports"][1] == 305


def pdsch_layers_pdu_nof_re(pdu):
    """Data REs per layer of one PdschLayersPdu record (host computation in the library); 0 on an invalid PDU."""
    a = np.ascontiguousarray(np.asarray(pdu, dtype=PdschLayersPdu).reshape(1))
    return int(lib().miphy_pdsch_layers_pdu_nof_re(a.ctypes.data_as(C.c_void_p)))


# Mirror miphy_pdsch_mod_mapped_job and miphy_pdsch_mapped_pdu: the layered records plus the place of the PRB list (mapping order) in the batch's
# uint16 list array; nof_prb = 0: no list, rb_mask ascending.
PdschModMappedJob = np.dtype([("layers", PdschModLayersJob), ("prb_list_offset", np.uint32), ("nof_prb", np.uint16), ("pad", np.uint16)], align=True)
assert PdschModMappedJob.itemsize == 296 and PdschModMappedJob.fields["prb_list_offset"][1] == 288 and PdschModMappedJob.fields["nof_prb"][1] == 292
PdschMappedPdu = np.dtype([("layers", PdschLayersPdu), ("prb_list_offset", np.uint32), ("nof_prb", np.uint16), ("pad", np.uint16)], align=True)
assert PdschMappedPdu.itemsize == 320 and PdschMappedPdu.fields["prb_list_offset"][1] == 312 and PdschMappedPdu.fields["nof_prb"][1] == 316
# Mirror miphy_pdsch_mod_codewords_job and miphy_pdsch_codewords_pdu: the mapped records (codeword / transport block 0 and everything the two share; the
# layers and ports inside them are ignored), nof_layers 1..8 with the grid port of each, and codeword / transport block 1, which exists from five layers.
PdschModCodewordsJob = np.dtype([("mapped", PdschModMappedJob), ("nof_layers", np.uint8), ("mod1", np.uint8), ("ports", np.uint8, 8), ("pad", np.uint8, 2),
                                 ("nof_bits1", np.uint32), ("cw1_offset", np.uint64)], align=True)
assert PdschModCodewordsJob.itemsize == 320 and PdschModCodewordsJob.fields["ports"][1] == 298 and PdschModCodewordsJob.fields["nof_bits1"][1] == 308
PdschCodewordsPdu = np.dtype([("mapped", PdschMappedPdu), ("nof_layers", np.uint8), ("ports", np.uint8, 8), ("bg1", np.uint8), ("rv1", np.uint8),
                              ("mod1", np.uint8), ("tb_bytes1", np.uint32), ("tb_offset1", np.uint64)], align=True)
assert PdschCodewordsPdu.itemsize == 344 and PdschCodewordsPdu.fields["bg1"][1] == 329 and PdschCodewordsPdu.fields["tb_bytes1"][1] == 332


def pdsch_mod_codewords_nof_re(job):
    """Data REs per layer of one PdschModCodewordsJob record (host computation in the library); 0 on an invalid job."""
    a = np.ascontiguousarray(np.asarray(job, dtype=PdschModCodewordsJob).reshape(1))
    return int(lib().miphy_pdsch_mod_codewords_nof_re(a.ctypes.data_as(C.c_void_p)))


def pdsch_codewords_pdu_nof_re(pdu):
    """Data REs per layer of one PdschCodewordsPdu record (host computation in the library); 0 on an invalid PDU."""
    a = np.ascontiguousarray(np.asarray(pdu, dtype=PdschCodewordsPdu).reshape(1))
    return int(lib().miphy_pdsch_codewords_pdu_nof_re(a.ctypes.data_as(C.c_void_p)))


# Mirrors miphy_precoding: nof_layers layers onto nof_ports antenna ports (grid port ports[a]) through one matrix per PRG of prg_size grid PRBs;
# W[g][a][ly] is cf_t entry weights_offset + (g nof_ports + a) nof_layers + ly of the call's weights.
Precoding = np.dtype([("nof_layers", np.uint8), ("nof_ports", np.uint8), ("ports", np.uint8, 16), ("prg_size", np.uint16), ("nof_prg", np.uint16),
                      ("pad0", np.uint16), ("weights_offset", np.uint32), ("pad1", np.uint32)], align=True)
assert Precoding.itemsize == 32 and Precoding.fields["prg_size"][1] == 18 and Precoding.fields["weights_offset"][1] == 24
# Mirrors miphy_precode_job: one matrix [port][layer], input [layer][in_stride], output [port][out_stride] (cf_t offsets and strides).
PrecodeJob = np.dtype([("nof_re", np.uint32), ("nof_layers", np.uint8), ("nof_ports", np.uint8), ("pad0", np.uint16), ("weights_offset", np.uint32),
                       ("pad1", np.uint32), ("in_offset", np.uint64), ("in_stride", np.uint64), ("out_offset", np.uint64), ("out_stride", np.uint64)], align=True)
assert PrecodeJob.itemsize == 48 and PrecodeJob.fields["in_offset"][1] == 16
# Mirror miphy_pdsch_mod_precoded_job, miphy_dmrs_pdsch_precoded_job and miphy_pdsch_precoded_pdu: the record without precoding, then the precoding.
PdschModPrecodedJob = np.dtype([("mapped", PdschModMappedJob), ("precoding", Precoding)], align=True)
DmrsPdschPrecodedJob = np.dtype([("base", DmrsPdschJob), ("precoding", Precoding)], align=True)
PdschPrecodedPdu = np.dtype([("mapped", PdschMappedPdu), ("precoding", Precoding)], align=True)
assert PdschModPrecodedJob.itemsize == 328 and DmrsPdschPrecodedJob.itemsize == 120 and PdschPrecodedPdu.itemsize == 352
# Mirrors miphy_vrb_to_prb.
VrbToPrb = np.dtype([("bundle_size", np.uint8), ("pad", np.uint8), ("align_rb", np.uint16), ("region_size_rb", np.uint16), ("first_prb", np.uint16)], align=True)
assert VrbToPrb.itemsize == 8


def vrb_to_prb_list(bundle_size, align_rb, region_size_rb, first_prb, vrbs=None, cap=None):
    """VRB-to-PRB mapping of TS 38.211 7.3.1.6 (miphy_vrb_to_prb_list, host computation in the library): the PRBs of the VRBs `vrbs` (any iterable
    of VRB numbers below 320; None: all of the region) in ascending VRB order, which is the mapping order of the mapped PDSCH entry points.
    Returns (uint16 list, the five words of its PRB mask). cap: entries the list may hold (default: 275). RuntimeError with "miphy error -1"
    where the library returns MIPHY_EINVAL."""
    m = np.zeros(1, dtype=VrbToPrb)
    m[0]["bundle_size"], m[0]["align_rb"], m[0]["region_size_rb"], m[0]["first_prb"] = bundle_size, align_rb, region_size_rb, first_prb
    vrb_mask = np.zeros(5, np.uint64)
    for v in (range(min(int(region_size_rb), 320)) if vrbs is None else vrbs):
        vrb_mask[int(v) >> 6] |= np.uint64(1) << np.uint64(int(v) & 63)
    cap = 275 if cap is None else int(cap)
    out, n, pm = np.zeros(max(cap, 1), np.uint16), C.c_uint32(0), np.zeros(5, np.uint64)
    check(lib().miphy_vrb_to_prb_list(m.ctypes.data_as(C.c_void_p), vrb_mask.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap, C.byref(n),
                                      pm.ctypes.data_as(C.c_void_p)))
    return out[:n.value].copy(), pm


# Mirrors miphy_csi_rs_job.
CsiRsJob = np.dtype([("slot_in_frame", np.uint32), ("scrambling_id", np.uint32), ("amplitude", np.float32), ("start_rb", np.uint16), ("nof_rb", np.uint16),
                     ("rb_begin", np.uint16), ("rb_end", np.uint16), ("rb_stride", np.uint16), ("grid_nof_prb", np.uint16), ("mapping_row", np.uint8),
                     ("cdm", np.uint8), ("freq_density", np.uint8), ("nof_ports", np.uint8), ("ports", np.uint8, 16), ("re_mask", np.uint16, 16),
                     ("symbol_mask", np.uint16, 16), ("grid_offset", np.uint64)], align=True)
assert CsiRsJob.itemsize == 120 and CsiRsJob.fields["grid_offset"][1] == 112, CsiRsJob.itemsize

# Mirrors miphy_pdcch_pdu.
PdcchPdu = np.dtype([("slot_in_frame", np.uint32), ("rnti", np.uint32), ("n_id_pdcch_data", np.uint32), ("n_rnti", np.uint32), ("n_id_pdcch_dmrs", np.uint32),
                     ("reference_point_k_rb", np.uint32), ("data_power_offset_dB", np.float32), ("dmrs_power_offset_dB", np.float32),
                     ("payload_size", np.uint16), ("aggregation_level", np.uint8), ("start_symbol", np.uint8), ("duration", np.uint8), ("port", np.uint8),
                     ("grid_nof_prb", np.uint16), ("rb_mask", np.uint64, 5), ("payload_offset", np.uint64), ("grid_offset", np.uint64),
                     ("work_offset", np.uint64)], align=True)
assert PdcchPdu.itemsize == 104 and PdcchPdu.fields["rb_mask"][1] == 40, PdcchPdu.itemsize

# Mirrors miphy_pusch_pdu.
PuschPdu = np.dtype([("numerology", np.uint32), ("slot_in_frame", np.uint32), ("rnti", np.uint32), ("n_id", np.uint32),
                     ("dmrs_scrambling_id", np.uint32), ("Nref", np.uint32), ("tb_bytes", np.uint32), ("harq_cb_index", np.uint32),
                     ("n_scid", np.uint8), ("mod", np.uint8), ("nof_rx_ports", np.uint8), ("start_symbol", np.uint8), ("nof_symbols", np.uint8),
                     ("bg", np.uint8), ("rv", np.uint8), ("new_data", np.uint8), ("rx_ports", np.uint8, 4), ("use_early_stop", np.uint8),
                     ("reserved0", np.uint8), ("nof_ldpc_iterations", np.uint16), ("dmrs_symbols_mask", np.uint16), ("grid_nof_prb", np.uint16),
                     ("pad", np.uint32), ("rb_mask", np.uint64, 5), ("grid_offset", np.uint64), ("tb_offset", np.uint64)], align=True)
assert PuschPdu.itemsize == 112 and PuschPdu.fields["rb_mask"][1] == 56, PuschPdu.itemsize

# Mirrors miphy_pusch_layers_pdu.
PuschLayersPdu = np.dtype([("base", PuschPdu), ("nof_tx_layers", np.uint8), ("reserved", np.uint8, 7)], align=True)
assert PuschLayersPdu.itemsize == 120 and PuschLayersPdu.fields["nof_tx_layers"][1] == 112, PuschLayersPdu.itemsize


# Mirrors miphy_pusch_mmse_pdu: a layered PDU through MMSE-IRC.
PuschMmsePdu = np.dtype([("base", PuschLayersPdu), ("loading", np.float32), ("prg_size", np.uint16), ("reserved", np.uint8, 2)], align=True)
assert PuschMmsePdu.itemsize == 128 and PuschMmsePdu.fields["loading"][1] == 120, PuschMmsePdu.itemsize


# Mirrors miphy_pusch_tp_pdu: a transform-precoded PUSCH.
PuschTpPdu = np.dtype([("base", PuschPdu), ("hopping", np.uint8), ("reserved", np.uint8, 7)], align=True)
assert PuschTpPdu.itemsize == 120 and PuschTpPdu.fields["hopping"][1] == 112, PuschTpPdu.itemsize


# Mirrors miphy_pusch_uci.
PuschUci = np.dtype([("nof_harq_ack_bits", np.uint32), ("nof_csi_part1_bits", np.uint32), ("nof_csi_part2_bits", np.uint32),
                     ("nof_enc_harq_ack_bits", np.uint32), ("nof_enc_csi_part1_bits", np.uint32), ("nof_enc_csi_part2_bits", np.uint32),
                     ("nof_harq_ack_rvd", np.uint32), ("has_codeword", np.uint32), ("harq_ack_offset", np.uint64), ("csi_part1_offset", np.uint64),
                     ("csi_part2_offset", np.uint64)], align=True)
assert PuschUci.itemsize == 56

# Mirrors miphy_uci_field_job; MIPHY_UCI_STATUS_* (srsran::uci_status).
UciFieldJob = np.dtype([("nof_bits", np.uint8), ("mod", np.uint8), ("reserved", np.uint16), ("nof_llr", np.uint32), ("llr_offset", np.uint64),
                        ("payload_offset", np.uint64)], align=True)
assert UciFieldJob.itemsize == 24
UCI_STATUS_UNKNOWN, UCI_STATUS_VALID, UCI_STATUS_INVALID = 0, 1, 2
# Mirrors miphy_uci_polar_job / miphy_uci_polar_info_t (polar-coded UCI fields of 12 to 1706 bits).
UciPolarJob = np.dtype([("nof_bits", np.uint16), ("reserved", np.uint16), ("nof_llr", np.uint32), ("llr_offset", np.uint64),
                        ("payload_offset", np.uint64)], align=True)
assert UciPolarJob.itemsize == 24
UciPolarInfo = np.dtype([("C", np.uint32), ("L", np.uint32), ("K_r", np.uint32), ("E_r", np.uint32), ("n", np.uint32), ("nPC", np.uint32)], align=True)
assert UciPolarInfo.itemsize == 24

# miphy_pucch_job / miphy_pucch_result (include/miphy.h)
PucchJob = np.dtype([("format", np.uint8), ("numerology", np.uint8), ("slot", np.uint16), ("nof_ports", np.uint8), ("start_symbol", np.uint8),
                     ("nof_symbols", np.uint8), ("intra_slot_hopping", np.uint8), ("bwp_start_rb", np.uint16), ("bwp_size_rb", np.uint16),
                     ("starting_prb", np.uint16), ("second_hop_prb", np.uint16), ("nof_prb", np.uint8), ("initial_cyclic_shift", np.uint8),
                     ("time_domain_occ", np.uint8), ("nof_harq_ack", np.uint8), ("nof_sr", np.uint8), ("nof_csi_part1", np.uint8),
                     ("nof_csi_part2", np.uint8), ("reserved0", np.uint8), ("n_id", np.uint16), ("n_id_0", np.uint16), ("rnti", np.uint16),
                     ("reserved1", np.uint16), ("grid_nprb", np.uint32), ("grid_offset", np.uint64), ("payload_offset", np.uint64),
                     ("llr_offset", np.uint64)], align=True)
assert PucchJob.itemsize == 64
PucchResult = np.dtype([("status", np.uint8), ("reserved", np.uint8, 3), ("detection_metric", np.float32), ("epre_db", np.float32),
                        ("rsrp_db", np.float32), ("sinr_db", np.float32), ("time_alignment_s", np.float32)], align=True)
assert PucchResult.itemsize == 24
# miphy_pucch_f34_job / miphy_pucch_f34_info_t (include/miphy.h)
PucchF34Job = np.dtype([("format", np.uint8), ("numerology", np.uint8), ("slot", np.uint16), ("nof_ports", np.uint8), ("start_symbol", np.uint8),
                        ("nof_symbols", np.uint8), ("intra_slot_hopping", np.uint8), ("bwp_start_rb", np.uint16), ("bwp_size_rb", np.uint16),
                        ("starting_prb", np.uint16), ("second_hop_prb", np.uint16), ("nof_prb", np.uint8), ("pi2_bpsk", np.uint8),
                        ("additional_dmrs", np.uint8), ("occ_length", np.uint8), ("occ_index", np.uint8), ("reserved0", np.uint8, 3),
                        ("nof_harq_ack", np.uint16), ("nof_sr", np.uint16), ("nof_csi_part1", np.uint16), ("nof_csi_part2", np.uint16),
                        ("n_id_hopping", np.uint16), ("n_id_scrambling", np.uint16), ("rnti", np.uint16), ("reserved1", np.uint16),
                        ("grid_nprb", np.uint32), ("reserved2", np.uint32), ("grid_offset", np.uint64), ("payload_offset", np.uint64),
                        ("llr_offset", np.uint64), ("est_offset", np.uint64)], align=True)
assert PucchF34Job.itemsize == 80
PucchF34Info = np.dtype([("dmrs_symbols_mask", np.uint32), ("nof_dmrs_symbols", np.uint32, 2), ("nof_data_symbols", np.uint32, 2), ("M", np.uint32),
                         ("E", np.uint32), ("polar", np.uint32)], align=True)
assert PucchF34Info.itemsize == 32


def pucch_f34_info(job):
    """What the PUCCH format 3 / 4 processor derives from one PucchF34Job record (host function, no device): a PucchF34Info record.
    Raises with the library's error code (-1 = MIPHY_EINVAL, -4 = MIPHY_EUNSUPP for format 3 on 2 PRBs) and the rule in the message."""
    j = np.ascontiguousarray(np.asarray(job, PucchF34Job).reshape(1))
    out = np.zeros(1, PucchF34Info)
    check(lib().miphy_pucch_f34_info(C.c_void_p(j.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out[0]


# miphy_pucch_f0_job / miphy_pucch_f0_info_t (include/miphy.h)
PucchF0Job = np.dtype([("format", np.uint8), ("numerology", np.uint8), ("slot", np.uint16), ("nof_ports", np.uint8), ("start_symbol", np.uint8),
                       ("nof_symbols", np.uint8), ("intra_slot_hopping", np.uint8), ("bwp_start_rb", np.uint16), ("bwp_size_rb", np.uint16),
                       ("starting_prb", np.uint16), ("second_hop_prb", np.uint16), ("initial_cyclic_shift", np.uint8), ("nof_harq_ack", np.uint8),
                       ("nof_sr", np.uint8), ("reserved0", np.uint8), ("used_shifts_mask", np.uint16), ("n_id", np.uint16), ("threshold", np.float32),
                       ("noise_var", np.float32), ("grid_nprb", np.uint32), ("reserved1", np.uint32), ("grid_offset", np.uint64),
                       ("payload_offset", np.uint64), ("energy_offset", np.uint64)], align=True)
assert PucchF0Job.itemsize == 64
PucchF0Info = np.dtype([("nof_hypotheses", np.uint32), ("shifts", np.uint8, 8), ("D", np.uint32), ("free_mask", np.uint32), ("F", np.uint32),
                        ("threshold", np.float32)], align=True)
assert PucchF0Info.itemsize == 28


def pucch_f0_info(job):
    """What the PUCCH format 0 detector derives from one PucchF0Job record (host function, no device): a PucchF0Info record -- the
    hypotheses' unhopped cyclic shifts in table order, D, the free shifts and the threshold the batch call would use. Raises with the
    library's error code (-1 = MIPHY_EINVAL) and the rule in the message."""
    j = np.ascontiguousarray(np.asarray(job, PucchF0Job).reshape(1))
    out = np.zeros(1, PucchF0Info)
    check(lib().miphy_pucch_f0_info(C.c_void_p(j.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out[0]


# miphy_srs_job / miphy_srs_info_t / miphy_srs_result (include/miphy.h)
SrsJob = np.dtype([("numerology", np.uint8), ("nof_rx_ports", np.uint8), ("slot", np.uint16), ("nof_tx_ports", np.uint8), ("start_symbol", np.uint8),
                   ("nof_symbols", np.uint8), ("comb_size", np.uint8), ("comb_offset", np.uint8), ("cyclic_shift", np.uint8), ("hopping", np.uint8),
                   ("prg_size", np.uint8), ("start_prb", np.uint16), ("nof_prb", np.uint16), ("n_id", np.uint16), ("reserved0", np.uint16),
                   ("grid_nprb", np.uint32), ("grid_offset", np.uint64), ("h_offset", np.uint64), ("pilots_offset", np.uint64)], align=True)
assert SrsJob.itemsize == 48
SrsInfo = np.dtype([("M", np.uint32), ("Q", np.uint32), ("P", np.uint32), ("G", np.uint32), ("nof_combs", np.uint32), ("cyclic_shifts", np.uint8, 4),
                    ("comb_offsets", np.uint8, 4), ("nof_h", np.uint32), ("max_delay_s", np.float32)], align=True)
assert SrsInfo.itemsize == 36
SrsResult = np.dtype([("h_wb", np.float32, (4, 4, 2)), ("noise_var", np.float32), ("epre_db", np.float32), ("rsrp_db", np.float32, 4),
                      ("sinr_db", np.float32), ("time_alignment_s", np.float32), ("reserved", np.uint32, 2)], align=True)
assert SrsResult.itemsize == 168


def srs_info(job):
    """What the SRS estimator derives from one SrsJob record (host function, no device): an SrsInfo record -- the sequence length M, the comb
    elements per PRG Q, the ports that share a comb P, the PRGs G, cyclic shift and comb offset per transmit port, the cf_t count of the job's
    estimate and the unambiguous delay range. Raises with the library's error code (-1 = MIPHY_EINVAL, -4 = MIPHY_EUNSUPP for M = 24) and the
    rule in the message."""
    j = np.ascontiguousarray(np.asarray(job, SrsJob).reshape(1))
    out = np.zeros(1, SrsInfo)
    check(lib().miphy_srs_info(C.c_void_p(j.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out[0]


# miphy_precoding_weights_ue / miphy_precoding_weights_job / miphy_precoding_weights_info_t (include/miphy.h)
PrecodingWeightsUe = np.dtype([("h_offset", np.uint64), ("weights_offset", np.uint32), ("metrics_offset", np.uint32), ("start_prb", np.uint16),
                               ("nof_prb", np.uint16), ("prg_size", np.uint8), ("nof_ue_ports", np.uint8), ("nof_layers", np.uint8),
                               ("reserved0", np.uint8)], align=True)
assert PrecodingWeightsUe.itemsize == 24
PrecodingWeightsJob = np.dtype([("nof_ues", np.uint8), ("nof_ports", np.uint8), ("prg_size", np.uint16), ("nof_prg", np.uint16), ("reserved0", np.uint16),
                                ("reg", np.float32), ("amplitude", np.float32), ("ue", PrecodingWeightsUe, 4)], align=True)
assert PrecodingWeightsJob.itemsize == 112
PrecodingWeightsInfo = np.dtype([("nof_layers", np.uint32), ("nof_weights", np.uint32, 4), ("nof_metrics", np.uint32, 4), ("max_srs_prg", np.uint32),
                                 ("wave_form", np.uint32)], align=True)
assert PrecodingWeightsInfo.itemsize == 44


def precoding_weights_info(job):
    """What miphy_precoding_weights_batch derives from one PrecodingWeightsJob record (host function, no device): a PrecodingWeightsInfo record --
    the layers of all UEs L, the cf_t and float counts of each UE's weights and metrics, the largest number of SRS PRGs of one UE under one
    output PRG, and whether the job takes the wave form. Raises with the library's error code (-1 = MIPHY_EINVAL) and the rule in the message."""
    j = np.ascontiguousarray(np.asarray(job, PrecodingWeightsJob).reshape(1))
    out = np.zeros(1, PrecodingWeightsInfo)
    check(lib().miphy_precoding_weights_info(C.c_void_p(j.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out[0]
# MIPHY_PRACH_FORMAT_*: PRACH_FORMATS.index("B4") is the format number of a PrachJob
PRACH_FORMATS = ("0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3")
# miphy_prach_job / miphy_prach_result / miphy_prach_preamble_result / miphy_prach_gen_job (include/miphy.h)
PrachJob = np.dtype([("format", np.uint32), ("ra_scs", np.uint32), ("root_sequence_index", np.uint32), ("zero_correlation_zone", np.uint32),
                     ("restricted_set", np.uint32), ("start_preamble_index", np.uint32), ("nof_preamble_indices", np.uint32),
                     ("idft_size", np.uint32), ("symbol_offset", np.uint32), ("preamble_offset", np.uint32)], align=True)
assert PrachJob.itemsize == 40
PrachResult = np.dtype([("rssi", np.float32), ("delay_n_maximum", np.uint32), ("n_cs", np.uint32), ("n_cs_limited", np.uint32)], align=True)
assert PrachResult.itemsize == 16
PrachPreambleResult = np.dtype([("peak_index", np.uint32), ("delay_n", np.int32), ("peak_power", np.float32), ("metric", np.float32),
                                ("detected", np.uint32)], align=True)
assert PrachPreambleResult.itemsize == 20
PrachGenJob = np.dtype([("format", np.uint32), ("root_sequence_index", np.uint32), ("zero_correlation_zone", np.uint32),
                        ("restricted_set", np.uint32), ("preamble_index", np.uint32), ("out_offset", np.uint32)], align=True)
assert PrachGenJob.itemsize == 24
# miphy_prach_demod_job / miphy_prach_demod_info_t (include/miphy.h)
PRACH_MAX_TD_OCCASIONS, PRACH_MAX_FD_OCCASIONS = 7, 8
PrachDemodJob = np.dtype([("format", np.uint32), ("pusch_scs", np.uint32), ("nof_td_occasions", np.uint32), ("nof_fd_occasions", np.uint32),
                          ("start_symbol", np.uint32), ("rb_offset", np.uint32), ("nof_prb_ul_grid", np.uint32), ("nof_samples", np.uint32),
                          ("samples_offset", np.uint64), ("buffer_offset", np.uint64), ("max_nof_fd_occasions", np.uint32),
                          ("max_nof_symbols", np.uint32)], align=True)
assert PrachDemodJob.itemsize == 56
PrachDemodInfo = np.dtype([("L", np.uint32), ("ra_scs_hz", np.uint32), ("dft_size", np.uint32), ("nof_symbols", np.uint32), ("K", np.uint32),
                           ("k_bar", np.uint32), ("nof_rb_ra", np.uint32), ("window_samples", np.uint32),
                           ("td_sample_offset", np.uint32, PRACH_MAX_TD_OCCASIONS), ("td_cp_samples", np.uint32, PRACH_MAX_TD_OCCASIONS),
                           ("k_start", np.uint32, PRACH_MAX_FD_OCCASIONS)], align=True)
assert PrachDemodInfo.itemsize == 120


def prach_demod_info(sampling_rate_hz, job):
    """What the PRACH demodulator derives from one PrachDemodJob record at a sampling rate (host function, no device): a PrachDemodInfo
    record. Raises with the library's error code (-1 = MIPHY_EINVAL where the reference asserts, -4 = MIPHY_EUNSUPP for a DFT size
    the device does not transform) in the message."""
    j = np.ascontiguousarray(np.asarray(job, PrachDemodJob).reshape(1))
    out = np.zeros(1, PrachDemodInfo)
    check(lib().miphy_prach_demod_info(int(sampling_rate_hz), C.c_void_p(j.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out[0]


def pusch_uci_field_jobs(pdus, uci):
    """UciFieldJob records of the present UCI fields of PuschPdu / PuschUci arrays over the uci_llr_out layout of pusch_process_batch_ex
    (host function). Returns (jobs, job_field) with job_field = 3 * pdu + field (0 HARQ-ACK, 1 CSI part 1, 2 CSI part 2)."""
    assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschPdu and isinstance(uci, np.ndarray) and uci.dtype == PuschUci
    assert pdus.size == uci.size
    pdus, uci = np.ascontiguousarray(pdus), np.ascontiguousarray(uci)
    jobs = np.zeros(max(1, 3 * pdus.size), UciFieldJob)
    field = np.zeros(jobs.size, np.uint32)
    cnt = C.c_uint32()
    check(lib().miphy_pusch_uci_field_jobs(C.c_void_p(pdus.ctypes.data), C.c_void_p(uci.ctypes.data), pdus.size, C.c_void_p(jobs.ctypes.data),
                                           C.c_void_p(field.ctypes.data), C.byref(cnt)))
    return jobs[:cnt.value].copy(), field[:cnt.value].copy()


def uci_polar_info(nof_bits, nof_llr):
    """The framing of a polar-coded UCI field of nof_bits bits received as nof_llr soft bits (host function, no device): a UciPolarInfo
    record. Raises with the library's error code (-1 = MIPHY_EINVAL) and the rule that refuses the field in the message."""
    out = np.zeros(1, UciPolarInfo)
    check(lib().miphy_uci_polar_info(int(nof_bits), int(nof_llr), C.c_void_p(out.ctypes.data)))
    return out[0]


def pusch_uci_jobs(pdus, uci):
    """pusch_uci_field_jobs for PDUs whose fields may be longer than 11 bits (host function): fields of 1..11 bits become UciFieldJob
    records, those of 12..1706 bits UciPolarJob records, all payloads packed into one buffer in (PDU, field) order. Returns
    (short_jobs, short_field, polar_jobs, polar_field) with *_field = 3 * pdu + field. Only `mod` of a PDU record is read: for
    PuschLayersPdu records pass pdus["base"]."""
    assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschPdu and isinstance(uci, np.ndarray) and uci.dtype == PuschUci
    assert pdus.size == uci.size
    pdus, uci = np.ascontiguousarray(pdus), np.ascontiguousarray(uci)
    sj, pj = np.zeros(max(1, 3 * pdus.size), UciFieldJob), np.zeros(max(1, 3 * pdus.size), UciPolarJob)
    sf, pf = np.zeros(sj.size, np.uint32), np.zeros(pj.size, np.uint32)
    ns, npol = C.c_uint32(), C.c_uint32()
    check(lib().miphy_pusch_uci_jobs(C.c_void_p(pdus.ctypes.data), C.c_void_p(uci.ctypes.data), pdus.size, C.c_void_p(sj.ctypes.data),
                                     C.c_void_p(sf.ctypes.data), C.byref(ns), C.c_void_p(pj.ctypes.data), C.c_void_p(pf.ctypes.data), C.byref(npol)))
    return sj[:ns.value].copy(), sf[:ns.value].copy(), pj[:npol.value].copy(), pf[:npol.value].copy()


class PolarCode(C.Structure):
    """Mirrors miphy_polar_code (the arguments of srsran::polar_code::set)."""
    _fields_ = [("K", C.c_uint32), ("E", C.c_uint32), ("nMax", C.c_uint32), ("ibil", C.c_uint32)]

    def info(self):
        n, N, npc = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().miphy_polar_code_info(C.byref(self), C.byref(n), C.byref(N), C.byref(npc)))
        return n.value, N.value, npc.value


# Mirrors miphy_pusch_tb_desc / miphy_pusch_result / miphy_pdsch_tb_desc / miphy_sch_segmentation.
PuschTbDesc = np.dtype([("bg", np.uint8), ("rv", np.uint8), ("mod", np.uint8), ("nof_layers", np.uint8), ("new_data", np.uint8),
                        ("use_early_stop", np.uint8), ("nof_ldpc_iterations", np.uint16), ("Nref", np.uint32),
                        ("nof_ch_symbols", np.uint32), ("tb_bytes", np.uint32), ("harq_cb_index", np.uint32),
                        ("llr_offset", np.uint64), ("tb_offset", np.uint64)], align=True)
assert PuschTbDesc.itemsize == 40
PuschResult = np.dtype([("tb_crc_ok", np.int32), ("nof_codeblocks_total", np.uint32), ("iters_min", np.uint32),
                        ("iters_max", np.uint32), ("iters_mean", np.float32), ("nof_decoded", np.uint32)], align=True)
assert PuschResult.itemsize == 24
PdschTbDesc = np.dtype([("bg", np.uint8), ("rv", np.uint8), ("mod", np.uint8), ("nof_layers", np.uint8), ("Nref", np.uint32),
                        ("nof_ch_symbols", np.uint32), ("tb_bytes", np.uint32), ("tb_offset", np.uint64),
                        ("codeword_offset", np.uint64)], align=True)
assert PdschTbDesc.itemsize == 32
HARQ_CB_STRIDE = 66 * 384
HARQ_MSG_STRIDE = 1056


class SchSegmentation(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("nof_cbs", "Z", "K", "N", "nof_filler_bits", "nof_tb_crc_bits", "nof_cb_crc_bits",
                                          "cb_info_bits", "zero_pad")]


def sch_segmentation(tb_bytes, bg):
    """Host-side segmentation parameters (ldpc::compute_nof_codeblocks / compute_lifting_size / compute_codeblock_size)."""
    s = SchSegmentation()
    check(lib().miphy_sch_segmentation_info(tb_bytes, bg, C.byref(s)))
    return s


# Mirrors miphy_pbch_msg.
PbchMsg = np.dtype([("N_id", np.uint32), ("ssb_idx", np.uint32), ("L_max", np.uint32), ("hrf", np.uint32), ("sfn", np.uint32),
                    ("k_ssb", np.uint32), ("payload", np.uint8, 32)], align=True)
assert PbchMsg.itemsize == 56
# Mirrors miphy_ssb_pdu.
SsbPdu = np.dtype([("msg", PbchMsg), ("ssb_first_subcarrier", np.uint32), ("ssb_first_symbol", np.uint32), ("beta_pss_dB", np.float32),
                   ("grid_nof_prb", np.uint16), ("nof_ports", np.uint8), ("ports", np.uint8, 4), ("pad", np.uint8), ("grid_offset", np.uint64)], align=True)
assert SsbPdu.itemsize == 88 and SsbPdu.fields["grid_offset"][1] == 80, SsbPdu.itemsize


# Mirrors miphy_ulsch_demux_job.
UlschDemuxJob = np.dtype([("mod", np.uint8), ("nof_layers", np.uint8), ("start_symbol", np.uint8), ("nof_symbols", np.uint8), ("dmrs_type", np.uint8),
                          ("nof_cdm_groups_without_data", np.uint8), ("dmrs_symbols_mask", np.uint16), ("nof_prb", np.uint16), ("reserved", np.uint16),
                          ("nof_harq_ack_rvd", np.uint32), ("nof_enc_harq_ack_bits", np.uint32), ("nof_enc_csi_part1_bits", np.uint32),
                          ("nof_enc_csi_part2_bits", np.uint32), ("nof_harq_ack_bits", np.uint32), ("nof_csi_part1_bits", np.uint32),
                          ("nof_csi_part2_bits", np.uint32), ("in_offset", np.uint64), ("sch_offset", np.uint64), ("harq_ack_offset", np.uint64),
                          ("csi_part1_offset", np.uint64), ("csi_part2_offset", np.uint64)], align=True)
assert UlschDemuxJob.itemsize == 80, UlschDemuxJob.itemsize


def ulsch_demux_sizes(job):
    """(codeword LLRs in, UL-SCH LLRs out) of a UlschDemuxJob record (host function)."""
    a, b = C.c_uint32(), C.c_uint32()
    j = np.ascontiguousarray(np.asarray(job).reshape(1))
    check(lib().miphy_ulsch_demux_sizes(C.c_void_p(j.ctypes.data), C.byref(a), C.byref(b)))
    return a.value, b.value


def ulsch_placeholders(job):
    """RE indices of the repetition placeholders (ulsch_demultiplex::get_placeholders), host function."""
    j = np.ascontiguousarray(np.asarray(job).reshape(1))
    out = np.zeros(275 * 12 * 14, np.uint16)
    n = C.c_uint32()
    check(lib().miphy_ulsch_placeholders(C.c_void_p(j.ctypes.data), C.c_void_p(out.ctypes.data), out.size, C.byref(n)))
    return out[:n.value].copy()


# MIPHY_POLAR_OP_* of miphy_polar_block_batch.
(POLAR_OP_ALLOCATE, POLAR_OP_ENCODE, POLAR_OP_RATE_MATCH, POLAR_OP_RATE_DEMATCH, POLAR_OP_DECODE, POLAR_OP_DEALLOCATE, POLAR_OP_INTERLEAVE_TX,
 POLAR_OP_INTERLEAVE_RX) = range(8)

# Mirrors miphy_equalizer_job.
EqualizerJob = np.dtype([("nof_re", np.uint32), ("nof_rx_ports", np.uint8), ("nof_tx_layers", np.uint8), ("reserved", np.uint8, 2), ("noise_var", np.float32),
                         ("tx_scaling", np.float32), ("ch_symbols_offset", np.uint64), ("ch_estimates_offset", np.uint64), ("eq_symbols_offset", np.uint64),
                         ("eq_noise_vars_offset", np.uint64)], align=True)
assert EqualizerJob.itemsize == 48, EqualizerJob.itemsize
# Mirrors miphy_equalizer_mmse_job.
EqualizerMmseJob = np.dtype([("base", EqualizerJob), ("cov_offset", np.uint64), ("re_per_cov", np.uint32), ("reserved", np.uint32)], align=True)
assert EqualizerMmseJob.itemsize == 64 and EqualizerMmseJob.fields["cov_offset"][1] == 48, EqualizerMmseJob.itemsize

# Mirrors miphy_crc_desc.
CrcDesc = np.dtype([("bit_offset", np.uint64), ("nbits", np.uint32), ("poly", np.uint32)], align=True)
assert CrcDesc.itemsize == 16


def check(rc):
    if rc != 0:
        raise RuntimeError("miphy error %d: %s" % (rc, lib().miphy_last_error().decode()))


def _stream_ptr(stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


def _dptr(t):
    """Device pointer of a torch tensor (must be a contiguous CUDA/HIP tensor)."""
    if not t.is_cuda:
        raise ValueError("miphy expects device (HBM-resident) tensors; there is no CPU path")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


class Context:
    """One per host thread / GPU (miphy_create)."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("miphy needs a HIP device (MI355X); no CPU fallback exists")
        self.device = device
        torch.cuda.set_device(device)
        h = C.c_void_p()
        check(lib().miphy_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().miphy_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _descs(descs, dtype):
        """descs: numpy structured array (host) or torch uint8 device tensor holding the same bytes."""
        import torch
        if isinstance(descs, np.ndarray):
            assert descs.dtype == dtype, (descs.dtype, dtype)
            descs = np.ascontiguousarray(descs)
            return descs, descs.size, C.c_void_p(descs.ctypes.data), 0
        assert descs.dtype == torch.uint8 and descs.numel() % dtype.itemsize == 0
        return descs, descs.numel() // dtype.itemsize, _dptr(descs), 1

    # ------------------------------------------------------------------ LDPC decoder
    def ldpc_decode_batch(self, descs, llr, out_bits, iters, stream=None, limits=None):
        """limits: optional (max_Z, max_in_len) for device-resident descriptors."""
        import torch
        descs, n, ptr, on_dev = self._descs(descs, LdpcDecDesc)
        assert iters.dtype == torch.int32 and iters.numel() >= n
        lim = None
        if limits is not None:
            lim = (C.c_uint32 * 2)(int(limits[0]), int(limits[1]))
        check(lib().miphy_ldpc_decode_batch(self.h, ptr, on_dev, n, _dptr(llr), _dptr(out_bits), _dptr(iters),
                                            lim, _stream_ptr(stream)))

    # ------------------------------------------------------------------ LDPC rate (de)matching, encoder, CRC
    def ldpc_rate_dematch_batch(self, descs, llr_in, softbuf, stream=None, max_E=None):
        """max_E: optional bound on the rate-matched length for device-resident descriptors."""
        descs, n, ptr, on_dev = self._descs(descs, LdpcRdmDesc)
        lim = (C.c_uint32 * 1)(int(max_E)) if max_E is not None else None
        check(lib().miphy_ldpc_rate_dematch_batch(self.h, ptr, on_dev, n, _dptr(llr_in), _dptr(softbuf), lim, _stream_ptr(stream)))

    def ldpc_rate_match_batch(self, descs, cb_in, out, stream=None):
        descs, n, ptr, on_dev = self._descs(descs, LdpcRdmDesc)
        check(lib().miphy_ldpc_rate_match_batch(self.h, ptr, on_dev, n, _dptr(cb_in), _dptr(out), _stream_ptr(stream)))

    def ldpc_encode_batch(self, descs, msg_in, cb_out, stream=None):
        descs, n, ptr, on_dev = self._descs(descs, LdpcEncDesc)
        check(lib().miphy_ldpc_encode_batch(self.h, ptr, on_dev, n, _dptr(msg_in), _dptr(cb_out), _stream_ptr(stream)))

    def crc_batch(self, descs, data, checksums, stream=None):
        descs, n, ptr, on_dev = self._descs(descs, CrcDesc)
        check(lib().miphy_crc_batch(self.h, ptr, on_dev, n, _dptr(data), _dptr(checksums), _stream_ptr(stream)))

    # ------------------------------------------------------------------ DFT / OFDM
    def dft_batch(self, size, inverse, n, x, out, stream=None):
        check(lib().miphy_dft_batch(self.h, size, int(inverse), n, _dptr(x), _dptr(out), _stream_ptr(stream)))

    def ofdm_demodulate_slots(self, cfg, jobs, samples, grid, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, OfdmJob)
        check(lib().miphy_ofdm_demodulate_slots(self.h, C.byref(cfg), ptr, on_dev, n, _dptr(samples), _dptr(grid), _stream_ptr(stream)))

    def ofdm_modulate_slots(self, cfg, jobs, grid, samples, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, OfdmJob)
        check(lib().miphy_ofdm_modulate_slots(self.h, C.byref(cfg), ptr, on_dev, n, _dptr(grid), _dptr(samples), _stream_ptr(stream)))

    # ------------------------------------------------------------------ PDSCH modulator / PDSCH DM-RS
    def pdsch_modulate_batch(self, jobs, codewords, grid, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, PdschModJob)
        check(lib().miphy_pdsch_modulate_batch(self.h, ptr, on_dev, n, _dptr(codewords), _dptr(grid), _stream_ptr(stream)))

    def dmrs_pdsch_map_batch(self, jobs, grid, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, DmrsPdschJob)
        check(lib().miphy_dmrs_pdsch_map_batch(self.h, ptr, on_dev, n, _dptr(grid), _stream_ptr(stream)))

    def pdsch_process_batch(self, pdus, tb_in, grid, stream=None):
        """pdsch_processor::process for a batch of PDUs (host descriptors): transport blocks -> REs of the resource grid."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PdschPdu
        pdus = np.ascontiguousarray(pdus)
        check(lib().miphy_pdsch_process_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, _dptr(tb_in), _dptr(grid), _stream_ptr(stream)))

    def pdsch_modulate_layers_batch(self, jobs, codewords, grid, stream=None):
        """One codeword on 1..4 layers (TS 38.211 7.3.1.3), layer ly on grid port ports[ly]; jobs on the host or on the device."""
        jobs, n, ptr, on_dev = self._descs(jobs, PdschModLayersJob)
        check(lib().miphy_pdsch_modulate_layers_batch(self.h, ptr, on_dev, n, _dptr(codewords), _dptr(grid), _stream_ptr(stream)))

    def pdsch_process_layers_batch(self, pdus, tb_in, grid, stream=None):
        """pdsch_process_batch for PDUs of one codeword on 1..4 layers (host descriptors): transport blocks -> REs of the named grid ports."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PdschLayersPdu
        pdus = np.ascontiguousarray(pdus)
        check(lib().miphy_pdsch_process_layers_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, _dptr(tb_in), _dptr(grid), _stream_ptr(stream)))

    @staticmethod
    def _host_or_device(a, on_dev, np_dtype, torch_dtypes, what):
        """(pointer, elements) of an array that lives where the jobs live: numpy of np_dtype, or a device tensor of one of torch_dtypes."""
        if on_dev:
            assert a is None or a.dtype in torch_dtypes, what
            return (_dptr(a), a.numel()) if a is not None and a.numel() else (None, 0)
        a = np.zeros(0, np_dtype) if a is None else np.ascontiguousarray(a)
        assert a.dtype == np_dtype, what
        return (C.c_void_p(a.ctypes.data), a.size) if a.size else (None, 0)

    def pdsch_modulate_mapped_batch(self, jobs, prb_lists, codewords, grid, stream=None):
        """pdsch_modulate_layers_batch with the PRBs of each job in the mapping order of its list (interleaved VRB-to-PRB mapping: vrb_to_prb_list).
        jobs and prb_lists live in the same place: a PdschModMappedJob array with a uint16 numpy array (None: no lists), or uint8 and int16 /
        uint16 device tensors holding the same bytes."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, PdschModMappedJob)
        lptr, nl = self._host_or_device(prb_lists, on_dev, np.uint16, (torch.int16, torch.uint16), "prb_lists")
        check(lib().miphy_pdsch_modulate_mapped_batch(self.h, ptr, on_dev, n, lptr, nl, _dptr(codewords), _dptr(grid), _stream_ptr(stream)))

    def pdsch_process_mapped_batch(self, pdus, prb_lists, tb_in, grid, stream=None):
        """pdsch_process_layers_batch for PDUs whose PRBs are mapped in the order of their lists (host descriptors, host uint16 lists or None)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PdschMappedPdu
        pdus = np.ascontiguousarray(pdus)
        lptr, nl = self._host_or_device(prb_lists, 0, np.uint16, (), "prb_lists")
        check(lib().miphy_pdsch_process_mapped_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, lptr, nl, _dptr(tb_in), _dptr(grid), _stream_ptr(stream)))

    def pdsch_modulate_codewords_batch(self, jobs, prb_lists, codewords, grid, stream=None):
        """pdsch_modulate_mapped_batch for one or two codewords on 1..8 layers (PdschModCodewordsJob; from five layers the job carries codeword 1 as
        well, TS 38.211 Table 7.3.1.3-1). jobs and prb_lists live in the same place, as there."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, PdschModCodewordsJob)
        lptr, nl = self._host_or_device(prb_lists, on_dev, np.uint16, (torch.int16, torch.uint16), "prb_lists")
        check(lib().miphy_pdsch_modulate_codewords_batch(self.h, ptr, on_dev, n, lptr, nl, _dptr(codewords), _dptr(grid), _stream_ptr(stream)))

    def pdsch_process_codewords_batch(self, pdus, prb_lists, tb_in, grid, stream=None):
        """pdsch_process_mapped_batch for PDUs of one or two transport blocks on 1..8 layers (host PdschCodewordsPdu records, host uint16 lists or None)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PdschCodewordsPdu
        pdus = np.ascontiguousarray(pdus)
        lptr, nl = self._host_or_device(prb_lists, 0, np.uint16, (), "prb_lists")
        check(lib().miphy_pdsch_process_codewords_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, lptr, nl, _dptr(tb_in), _dptr(grid), _stream_ptr(stream)))

    # ------------------------------------------------------------------ precoding: layers to antenna ports through per-PRG weights
    def channel_precode_batch(self, jobs, weights, x, out, stream=None):
        """channel_precoder::apply_precoding for a batch of PrecodeJob: out[a][i] = sum_ly W[a][ly] x[ly][i]. jobs and weights live in the same place: a
        PrecodeJob array with a complex64 numpy array, or uint8 and complex64 device tensors; x and out are complex64 device tensors."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, PrecodeJob)
        wptr, nw = self._host_or_device(weights, on_dev, np.complex64, (torch.complex64,), "weights")
        check(lib().miphy_channel_precode_batch(self.h, ptr, on_dev, n, wptr, nw, _dptr(x), _dptr(out), _stream_ptr(stream)))

    def pdsch_modulate_precoded_batch(self, jobs, prb_lists, weights, codewords, grid, stream=None):
        """pdsch_modulate_mapped_batch whose data REs go through the per-PRG matrices of each job's precoding onto its antenna ports. jobs, prb_lists
        (None: no lists) and weights live in the same place: PdschModPrecodedJob / uint16 / complex64 numpy arrays, or uint8 / int16 / complex64
        device tensors."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, PdschModPrecodedJob)
        lptr, nl = self._host_or_device(prb_lists, on_dev, np.uint16, (torch.int16, torch.uint16), "prb_lists")
        wptr, nw = self._host_or_device(weights, on_dev, np.complex64, (torch.complex64,), "weights")
        check(lib().miphy_pdsch_modulate_precoded_batch(self.h, ptr, on_dev, n, lptr, nl, wptr, nw, _dptr(codewords), _dptr(grid), _stream_ptr(stream)))

    def dmrs_pdsch_map_precoded_batch(self, jobs, weights, grid, stream=None):
        """dmrs_pdsch_map_batch for the DM-RS ports of one codeword behind a precoding (DmrsPdschPrecodedJob; weights where the jobs are)."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, DmrsPdschPrecodedJob)
        wptr, nw = self._host_or_device(weights, on_dev, np.complex64, (torch.complex64,), "weights")
        check(lib().miphy_dmrs_pdsch_map_precoded_batch(self.h, ptr, on_dev, n, wptr, nw, _dptr(grid), _stream_ptr(stream)))

    def pdsch_process_precoded_batch(self, pdus, prb_lists, weights, tb_in, grid, stream=None):
        """pdsch_process_mapped_batch with precoding (host PdschPrecodedPdu records, host uint16 lists or None, host complex64 weights)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PdschPrecodedPdu
        pdus = np.ascontiguousarray(pdus)
        lptr, nl = self._host_or_device(prb_lists, 0, np.uint16, (), "prb_lists")
        wptr, nw = self._host_or_device(weights, 0, np.complex64, (), "weights")
        check(lib().miphy_pdsch_process_precoded_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, lptr, nl, wptr, nw, _dptr(tb_in), _dptr(grid),
                                                       _stream_ptr(stream)))

    def csi_rs_map_batch(self, jobs, grid, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, CsiRsJob)
        check(lib().miphy_csi_rs_map_batch(self.h, ptr, on_dev, n, _dptr(grid), _stream_ptr(stream)))

    def ssb_process_batch(self, pdus, grid, stream=None):
        """ssb_processor::process (after the position look-up) for a batch of SS/PBCH blocks (host descriptors)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == SsbPdu
        pdus = np.ascontiguousarray(pdus)
        check(lib().miphy_ssb_process_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, _dptr(grid), _stream_ptr(stream)))

    def pdcch_process_batch(self, pdus, payloads, grid, stream=None):
        """pdcch_processor::process (after the CCE-to-PRB mapping) for a batch of PDUs (host descriptors): DCI payload bits -> grid REs."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PdcchPdu
        pdus = np.ascontiguousarray(pdus)
        check(lib().miphy_pdcch_process_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, _dptr(payloads), _dptr(grid), _stream_ptr(stream)))

    # ------------------------------------------------------------------ Open Fronthaul IQ (de)compression (U-plane payloads <-> grid rows)
    def ofh_iq_decompress_batch(self, jobs, payload, grid, simd_arithmetic=True, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, OfhIqJob)
        check(lib().miphy_ofh_iq_decompress_batch(self.h, ptr, on_dev, n, _dptr(payload), _dptr(grid), int(simd_arithmetic), _stream_ptr(stream)))

    def ofh_iq_compress_batch(self, jobs, grid, payload, iq_scaling=1.0, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, OfhIqJob)
        check(lib().miphy_ofh_iq_compress_batch(self.h, ptr, on_dev, n, _dptr(grid), float(iq_scaling), _dptr(payload), _stream_ptr(stream)))

    # ------------------------------------------------------------------ PUSCH demodulator (equalise + soft-demap + descramble)
    def pusch_demodulate_batch_ex(self, jobs, grid, ce, scalars, llr, placeholders=None, evm_sums=None, stream=None):
        """With the repetition placeholders (device uint16) and / or the per-symbol EVM sums (device float32, 14 per job at evm_offset)."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodJob)
        check(lib().miphy_pusch_demodulate_batch_ex(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(llr),
                                                    _dptr(placeholders) if placeholders is not None else None,
                                                    _dptr(evm_sums) if evm_sums is not None else None, _stream_ptr(stream)))

    def pusch_demodulate_batch(self, jobs, grid, ce, scalars, llr, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodJob)
        check(lib().miphy_pusch_demodulate_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(llr), _stream_ptr(stream)))

    # ------------------------------------------------------------------ DM-RS PUSCH channel estimator
    def dmrs_pusch_estimate_batch(self, jobs, grid, ce, scalars, stream=None, max_ports=0, max_layers=0):
        """max_ports / max_layers: optional bound for device-resident jobs (sizes the launch; 0 = unknown)."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschChestJob)
        if on_dev:
            on_dev |= (int(max_ports) << 8) | (int(max_layers) << 12)
        check(lib().miphy_dmrs_pusch_estimate_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _stream_ptr(stream)))

    def dmrs_pusch_estimate_layers_batch(self, jobs, grid, ce, scalars, stream=None, max_ports=0, max_layers=0):
        """The estimator that separates the layers of a CDM group (PUSCH on 1..4 layers): jobs, outputs and hints as dmrs_pusch_estimate_batch."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschChestJob)
        if on_dev:
            on_dev |= (int(max_ports) << 8) | (int(max_layers) << 12)
        check(lib().miphy_dmrs_pusch_estimate_layers_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _stream_ptr(stream)))

    def dmrs_pusch_estimate_cfo_batch(self, jobs, grid, ce, scalars, cfo, stream=None, max_ports=0, max_layers=0):
        """The layered estimator with the carrier frequency offset estimated from the DM-RS symbols and compensated (PuschChestCfoJob records,
        ce_compact = 0: the estimate is written per symbol; cfo: device float32, {cfo_hz, rho} per job at cfo_offset); hints as dmrs_pusch_estimate_batch."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschChestCfoJob)
        if on_dev:
            on_dev |= (int(max_ports) << 8) | (int(max_layers) << 12)
        check(lib().miphy_dmrs_pusch_estimate_cfo_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(cfo), _stream_ptr(stream)))

    def dmrs_pusch_estimate_tv_batch(self, jobs, grid, ce, scalars, cfo, var, stream=None, max_ports=0, max_layers=0):
        """dmrs_pusch_estimate_cfo_batch for a channel that changes within the slot (PuschChestTvJob records): the fits of the DM-RS symbols are kept apart
        and interpolated in time (time_mode); var: device float32, the variation of every (port, layer) at var_offset; hints as dmrs_pusch_estimate_batch."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschChestTvJob)
        if on_dev:
            on_dev |= (int(max_ports) << 8) | (int(max_layers) << 12)
        check(lib().miphy_dmrs_pusch_estimate_tv_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(cfo), _dptr(var), _stream_ptr(stream)))

    def pusch_noise_covariance_batch(self, jobs, grid, cov, stream=None, max_ports=0, max_layers=0):
        """Noise-plus-interference covariance per PRG from the DM-RS residuals (PuschNcovJob records; cov: device complex64); hints as
        dmrs_pusch_estimate_batch."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschNcovJob)
        if on_dev:
            on_dev |= (int(max_ports) << 8) | (int(max_layers) << 12)
        check(lib().miphy_pusch_noise_covariance_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(cov), _stream_ptr(stream)))

    def port_channel_estimate_batch(self, jobs, grid, pilots, ce, scalars, stream=None):
        """port_channel_estimator::compute: pilots given by the caller (device complex64), optional intra-slot hopping."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschChestJob)
        check(lib().miphy_port_channel_estimate_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(pilots), _dptr(ce), _dptr(scalars), _stream_ptr(stream)))

    # ------------------------------------------------------------------ polar chains / PDCCH encoder
    def polar_encode_batch(self, code, n, msg, rm_out, allocated_tap=None, encoded_tap=None, stream=None):
        check(lib().miphy_polar_encode_batch(self.h, C.byref(code), n, _dptr(msg), _dptr(rm_out),
                                             _dptr(allocated_tap) if allocated_tap is not None else None,
                                             _dptr(encoded_tap) if encoded_tap is not None else None, _stream_ptr(stream)))

    def polar_decode_batch(self, code, n, llr, msg_out, dematched_tap=None, decoded_u_tap=None, stream=None):
        check(lib().miphy_polar_decode_batch(self.h, C.byref(code), n, _dptr(llr), _dptr(msg_out),
                                             _dptr(dematched_tap) if dematched_tap is not None else None,
                                             _dptr(decoded_u_tap) if decoded_u_tap is not None else None, _stream_ptr(stream)))

    def pdcch_encode_batch(self, A, E, n, payload, rnti, out, stream=None):
        check(lib().miphy_pdcch_encode_batch(self.h, A, E, n, _dptr(payload), _dptr(rnti), _dptr(out), _stream_ptr(stream)))

    # ------------------------------------------------------------------ transport-block level shared channel
    def pusch_decode_batch(self, tbs, llrs, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, stream=None):
        """tbs: numpy PuschTbDesc array (host). results: torch uint8 tensor of n * PuschResult.itemsize bytes."""
        assert isinstance(tbs, np.ndarray) and tbs.dtype == PuschTbDesc
        tbs = np.ascontiguousarray(tbs)
        check(lib().miphy_pusch_decode_batch(self.h, C.c_void_p(tbs.ctypes.data), tbs.size, _dptr(llrs), _dptr(harq_softbits),
                                             _dptr(harq_msgs), _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _stream_ptr(stream)))

    def ulsch_demultiplex_batch(self, jobs, llr_in, sch, harq_ack, csi1, csi2, stream=None):
        assert isinstance(jobs, np.ndarray) and jobs.dtype == UlschDemuxJob
        jobs = np.ascontiguousarray(jobs)
        check(lib().miphy_ulsch_demultiplex_batch(self.h, C.c_void_p(jobs.ctypes.data), jobs.size, _dptr(llr_in), _dptr(sch), _dptr(harq_ack),
                                                  _dptr(csi1), _dptr(csi2), _stream_ptr(stream)))

    def channel_equalize_batch(self, jobs, ch_symbols, ch_estimates, eq_symbols, eq_noise_vars, stream=None):
        """channel_equalizer::equalize (zero forcing) for a batch of EqualizerJob records."""
        jobs, n, ptr, on_dev = self._descs(jobs, EqualizerJob)
        check(lib().miphy_channel_equalize_batch(self.h, ptr, on_dev, n, _dptr(ch_symbols), _dptr(ch_estimates), _dptr(eq_symbols), _dptr(eq_noise_vars),
                                                 _stream_ptr(stream)))

    def channel_equalize_layers_batch(self, jobs, ch_symbols, ch_estimates, eq_symbols, eq_noise_vars, stream=None):
        """Zero forcing of 1..4 layers on at least as many (at most 4) receive ports for a batch of EqualizerJob records."""
        jobs, n, ptr, on_dev = self._descs(jobs, EqualizerJob)
        check(lib().miphy_channel_equalize_layers_batch(self.h, ptr, on_dev, n, _dptr(ch_symbols), _dptr(ch_estimates), _dptr(eq_symbols),
                                                        _dptr(eq_noise_vars), _stream_ptr(stream)))

    def channel_equalize_mmse_batch(self, jobs, ch_symbols, ch_estimates, cov, eq_symbols, eq_noise_vars, stream=None):
        """MMSE-IRC of 1..4 layers on at least as many (at most 4) receive ports for a batch of EqualizerMmseJob records (cov: device complex64)."""
        jobs, n, ptr, on_dev = self._descs(jobs, EqualizerMmseJob)
        check(lib().miphy_channel_equalize_mmse_batch(self.h, ptr, on_dev, n, _dptr(ch_symbols), _dptr(ch_estimates), _dptr(cov), _dptr(eq_symbols),
                                                      _dptr(eq_noise_vars), _stream_ptr(stream)))

    def pusch_demodulate_layers_batch(self, jobs, grid, ce, scalars, llr, stream=None):
        """PUSCH demodulator for one codeword on 1..4 transmit layers: a batch of PuschDemodLayersJob records."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodLayersJob)
        check(lib().miphy_pusch_demodulate_layers_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(llr), _stream_ptr(stream)))

    def pusch_demodulate_layers_batch_ex(self, jobs, grid, ce, scalars, llr, placeholders=None, evm_sums=None, stream=None):
        """pusch_demodulate_layers_batch with the repetition placeholders (device uint16: resource element indices as ulsch_placeholders gives them
        for the job's layer count) and / or the per-symbol EVM sums (device float32, 14 per job at evm_offset, summed over the layers)."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodLayersJob)
        check(lib().miphy_pusch_demodulate_layers_batch_ex(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(llr),
                                                           _dptr(placeholders) if placeholders is not None else None,
                                                           _dptr(evm_sums) if evm_sums is not None else None, _stream_ptr(stream)))

    def pusch_demodulate_layers_mmse_batch(self, jobs, grid, ce, cov, llr, scalars=None, stream=None):
        """pusch_demodulate_layers_batch with MMSE-IRC in place of zero forcing: a batch of PuschDemodMmseJob records, cov: device complex64
        [PRG][P][P] per job. The scalars are not read."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodMmseJob)
        check(lib().miphy_pusch_demodulate_layers_mmse_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars) if scalars is not None else None,
                                                             _dptr(cov), _dptr(llr), _stream_ptr(stream)))

    def pusch_demodulate_layers_mmse_batch_ex(self, jobs, grid, ce, cov, llr, placeholders=None, evm_sums=None, scalars=None, stream=None):
        """pusch_demodulate_layers_mmse_batch with the placeholders and / or EVM sums of pusch_demodulate_layers_batch_ex."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodMmseJob)
        check(lib().miphy_pusch_demodulate_layers_mmse_batch_ex(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars) if scalars is not None else None,
                                                                _dptr(cov), _dptr(llr), _dptr(placeholders) if placeholders is not None else None,
                                                                _dptr(evm_sums) if evm_sums is not None else None, _stream_ptr(stream)))

    # ------------------------------------------------------------------ PUSCH with transform precoding (DFT-s-OFDM)
    def transform_deprecode_batch(self, jobs, eq_symbols, eq_noise_vars, out_symbols, out_noise_var, stream=None):
        """The de-precoding IDFT of M = 12 N_PRB points and the mean noise variance per row: a batch of TransformDeprecodeJob records."""
        jobs, n, ptr, on_dev = self._descs(jobs, TransformDeprecodeJob)
        check(lib().miphy_transform_deprecode_batch(self.h, ptr, on_dev, n, _dptr(eq_symbols), _dptr(eq_noise_vars), _dptr(out_symbols),
                                                    _dptr(out_noise_var), _stream_ptr(stream)))

    def pusch_demodulate_tp_batch(self, jobs, grid, ce, scalars, llr, stream=None):
        """PUSCH demodulator for a transform-precoded transmission: a batch of PuschDemodJob records (contiguous allocation of 2^a 3^b 5^c PRBs,
        DM-RS type 1, two CDM groups without data)."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodJob)
        check(lib().miphy_pusch_demodulate_tp_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(llr), _stream_ptr(stream)))

    def pusch_demodulate_tp_batch_ex(self, jobs, grid, ce, scalars, llr, placeholders=None, evm_sums=None, stream=None):
        """pusch_demodulate_tp_batch with the repetition placeholders (device uint16) and / or the per-symbol EVM sums (device float32, 14 per job at
        evm_offset, over the de-precoded symbols)."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschDemodJob)
        check(lib().miphy_pusch_demodulate_tp_batch_ex(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _dptr(llr),
                                                       _dptr(placeholders) if placeholders is not None else None,
                                                       _dptr(evm_sums) if evm_sums is not None else None, _stream_ptr(stream)))

    def dmrs_pusch_tp_pilots_batch(self, jobs, pilots, stream=None):
        """The low-PAPR DM-RS of a batch of PuschChestTpJob records, [DM-RS symbol][6 N_PRB] complex64 at each job's pilots_offset."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschChestTpJob)
        check(lib().miphy_dmrs_pusch_tp_pilots_batch(self.h, ptr, on_dev, n, _dptr(pilots), _stream_ptr(stream)))

    def dmrs_pusch_estimate_tp_batch(self, jobs, grid, ce, scalars, stream=None, max_ports=0):
        """DM-RS estimator of a transform-precoded PUSCH: jobs PuschChestTpJob, outputs and the port hint as dmrs_pusch_estimate_batch."""
        jobs, n, ptr, on_dev = self._descs(jobs, PuschChestTpJob)
        if on_dev:
            on_dev |= int(max_ports) << 8
        check(lib().miphy_dmrs_pusch_estimate_tp_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(ce), _dptr(scalars), _stream_ptr(stream)))

    def pusch_process_tp_batch(self, pdus, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, stream=None):
        """A transform-precoded PUSCH. pdus: numpy PuschTpPdu array (host); results and scalars (float32 n x 20) as pusch_process_batch."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschTpPdu
        pdus = np.ascontiguousarray(pdus)
        check(lib().miphy_pusch_process_tp_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, _dptr(grid), _dptr(harq_softbits), _dptr(harq_msgs),
                                                 _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars), _stream_ptr(stream)))

    def pusch_process_tp_batch_ex(self, pdus, uci, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, uci_llr, evm, stream=None):
        """pusch_process_tp_batch for PDUs with multiplexed UCI (uci: numpy PuschUci array or None) and the EVM (evm: float32 device tensor of n or
        None). The field jobs behind it: pusch_uci_jobs(pdus["base"], uci)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschTpPdu
        pdus = np.ascontiguousarray(pdus)
        up = None
        if uci is not None:
            assert isinstance(uci, np.ndarray) and uci.dtype == PuschUci and uci.size == pdus.size
            uci = np.ascontiguousarray(uci)
            up = C.c_void_p(uci.ctypes.data)
        check(lib().miphy_pusch_process_tp_batch_ex(self.h, C.c_void_p(pdus.ctypes.data), up, pdus.size, _dptr(grid), _dptr(harq_softbits),
                                                    _dptr(harq_msgs), _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars),
                                                    _dptr(uci_llr) if uci_llr is not None else None, _dptr(evm) if evm is not None else None,
                                                    _stream_ptr(stream)))

    def polar_block_batch(self, code, op, param, n, x, out, stream=None):
        check(lib().miphy_polar_block_batch(self.h, C.byref(code) if code is not None else None, op, param, n, _dptr(x), _dptr(out), _stream_ptr(stream)))

    def ofdm_demodulate_symbols(self, cfg, jobs, samples, grid, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, OfdmJob)
        check(lib().miphy_ofdm_demodulate_symbols(self.h, C.byref(cfg), ptr, on_dev, n, _dptr(samples), _dptr(grid), _stream_ptr(stream)))

    def ofdm_modulate_symbols(self, cfg, jobs, grid, samples, stream=None):
        jobs, n, ptr, on_dev = self._descs(jobs, OfdmJob)
        check(lib().miphy_ofdm_modulate_symbols(self.h, C.byref(cfg), ptr, on_dev, n, _dptr(grid), _dptr(samples), _stream_ptr(stream)))

    def pusch_decode_plan(self, tbs):
        """Prepared miphy_pusch_decode_batch (descriptors uploaded once): returns a PuschDecodePlan."""
        return PuschDecodePlan(self, tbs)

    def pusch_process_batch(self, pdus, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, stream=None):
        """pdus: numpy PuschPdu array (host). results: torch uint8 tensor of n * PuschResult.itemsize bytes; scalars: float32 n x 20."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschPdu
        pdus = np.ascontiguousarray(pdus)
        check(lib().miphy_pusch_process_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, _dptr(grid), _dptr(harq_softbits), _dptr(harq_msgs),
                                              _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars), _stream_ptr(stream)))

    def pusch_process_layers_batch(self, pdus, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, stream=None):
        """One codeword on 1..4 layers. pdus: numpy PuschLayersPdu array (host); results as pusch_process_batch; scalars: float32 n x 80,
        [rx port][layer][5] of PDU i at 80 i + 5 (port * nof_tx_layers + layer)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschLayersPdu
        pdus = np.ascontiguousarray(pdus)
        check(lib().miphy_pusch_process_layers_batch(self.h, C.c_void_p(pdus.ctypes.data), pdus.size, _dptr(grid), _dptr(harq_softbits), _dptr(harq_msgs),
                                                     _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars), _stream_ptr(stream)))

    def pusch_process_layers_mmse_batch(self, pdus, uci, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, uci_llr=None, evm=None, stream=None):
        """pusch_process_layers_batch_ex with MMSE-IRC (host PuschMmsePdu records): the covariance estimator behind the layered estimator, the MMSE
        demodulator in place of the zero-forcing one."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschMmsePdu
        pdus = np.ascontiguousarray(pdus)
        up = None
        if uci is not None:
            assert isinstance(uci, np.ndarray) and uci.dtype == PuschUci and uci.size == pdus.size
            uci = np.ascontiguousarray(uci)
            up = C.c_void_p(uci.ctypes.data)
        check(lib().miphy_pusch_process_layers_mmse_batch(self.h, C.c_void_p(pdus.ctypes.data), up, pdus.size, _dptr(grid), _dptr(harq_softbits),
                                                          _dptr(harq_msgs), _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars),
                                                          _dptr(uci_llr) if uci_llr is not None else None, _dptr(evm) if evm is not None else None,
                                                          _stream_ptr(stream)))

    def pusch_process_layers_cfo_batch(self, pdus, uci, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, uci_llr, evm, cfo, stream=None):
        """pusch_process_layers_batch_ex with dmrs_pusch_estimate_cfo_batch in front and a per-symbol estimate behind it; cfo: device float32 [n][2],
        {cfo_hz, rho} per PDU."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschLayersPdu
        pdus = np.ascontiguousarray(pdus)
        up = None
        if uci is not None:
            assert isinstance(uci, np.ndarray) and uci.dtype == PuschUci and uci.size == pdus.size
            uci = np.ascontiguousarray(uci)
            up = C.c_void_p(uci.ctypes.data)
        check(lib().miphy_pusch_process_layers_cfo_batch(self.h, C.c_void_p(pdus.ctypes.data), up, pdus.size, _dptr(grid), _dptr(harq_softbits),
                                                         _dptr(harq_msgs), _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars),
                                                         _dptr(uci_llr) if uci_llr is not None else None, _dptr(evm) if evm is not None else None,
                                                         _dptr(cfo), _stream_ptr(stream)))

    def pusch_process_layers_tv_batch(self, pdus, uci, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, uci_llr, evm, cfo, time_mode, var,
                                      stream=None):
        """pusch_process_layers_cfo_batch with dmrs_pusch_estimate_tv_batch in front (time_mode: TIME_INTERPOLATE or TIME_LINE); var: device float32 [n][16],
        the variation of (port, layer) of every PDU at port * nof_tx_layers + layer."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschLayersPdu
        pdus = np.ascontiguousarray(pdus)
        up = None
        if uci is not None:
            assert isinstance(uci, np.ndarray) and uci.dtype == PuschUci and uci.size == pdus.size
            uci = np.ascontiguousarray(uci)
            up = C.c_void_p(uci.ctypes.data)
        check(lib().miphy_pusch_process_layers_tv_batch(self.h, C.c_void_p(pdus.ctypes.data), up, pdus.size, _dptr(grid), _dptr(harq_softbits),
                                                        _dptr(harq_msgs), _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars),
                                                        _dptr(uci_llr) if uci_llr is not None else None, _dptr(evm) if evm is not None else None,
                                                        _dptr(cfo), int(time_mode), _dptr(var), _stream_ptr(stream)))

    def pusch_process_layers_batch_ex(self, pdus, uci, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, uci_llr, evm, stream=None):
        """pusch_process_layers_batch for PDUs with multiplexed UCI (uci: numpy PuschUci array or None) and the EVM (evm: float32 device tensor of n or
        None). The field jobs behind it: pusch_uci_jobs(pdus["base"], uci)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschLayersPdu
        pdus = np.ascontiguousarray(pdus)
        up = None
        if uci is not None:
            assert isinstance(uci, np.ndarray) and uci.dtype == PuschUci and uci.size == pdus.size
            uci = np.ascontiguousarray(uci)
            up = C.c_void_p(uci.ctypes.data)
        check(lib().miphy_pusch_process_layers_batch_ex(self.h, C.c_void_p(pdus.ctypes.data), up, pdus.size, _dptr(grid), _dptr(harq_softbits),
                                                        _dptr(harq_msgs), _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars),
                                                        _dptr(uci_llr) if uci_llr is not None else None, _dptr(evm) if evm is not None else None,
                                                        _stream_ptr(stream)))

    def pusch_process_batch_ex(self, pdus, uci, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars, uci_llr, evm, stream=None):
        """PDUs with multiplexed UCI (uci: numpy PuschUci array or None) and the EVM (evm: float32 device tensor of n or None)."""
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PuschPdu
        pdus = np.ascontiguousarray(pdus)
        up = None
        if uci is not None:
            assert isinstance(uci, np.ndarray) and uci.dtype == PuschUci and uci.size == pdus.size
            uci = np.ascontiguousarray(uci)
            up = C.c_void_p(uci.ctypes.data)
        check(lib().miphy_pusch_process_batch_ex(self.h, C.c_void_p(pdus.ctypes.data), up, pdus.size, _dptr(grid), _dptr(harq_softbits), _dptr(harq_msgs),
                                                 _dptr(harq_crc_ok), _dptr(tb_out), _dptr(results), _dptr(scalars),
                                                 _dptr(uci_llr) if uci_llr is not None else None, _dptr(evm) if evm is not None else None,
                                                 _stream_ptr(stream)))

    def uci_decode_batch(self, jobs, llr, payload, status, stream=None):
        """Short-block detection of UCI fields (jobs: numpy UciFieldJob array, or a uint8 device tensor holding the same bytes): llr int8,
        payload uint8 (one bit per byte) and status uint8 (one per job) device tensors."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, UciFieldJob)
        assert llr.dtype == torch.int8 and payload.dtype == torch.uint8 and status.dtype == torch.uint8
        check(lib().miphy_uci_decode_batch(self.h, ptr, on_dev, n, _dptr(llr), _dptr(payload), _dptr(status), _stream_ptr(stream)))

    def uci_polar_decode_batch(self, jobs, llr, payload, status, stream=None):
        """Polar-coded UCI fields of 12 to 1706 bits (jobs: numpy UciPolarJob array, HOST memory only): llr int8, payload uint8 (one bit
        per byte, nof_bits bytes per job) and status uint8 (one per job) device tensors. Only enqueues."""
        import torch
        assert isinstance(jobs, np.ndarray) and jobs.dtype == UciPolarJob, "uci_polar_decode_batch takes host jobs"
        jobs = np.ascontiguousarray(jobs)
        assert llr.dtype == torch.int8 and payload.dtype == torch.uint8 and status.dtype == torch.uint8
        if jobs.size:  # the extents the kernel may touch lie inside the tensors (the library sees raw pointers)
            assert (jobs["llr_offset"].astype(np.int64) + jobs["nof_llr"].astype(np.int64)).max() <= llr.numel(), "soft bits outside `llr`"
            assert (jobs["payload_offset"].astype(np.int64) + jobs["nof_bits"].astype(np.int64)).max() <= payload.numel(), "payload outside `payload`"
            assert status.numel() >= jobs.size
        check(lib().miphy_uci_polar_decode_batch(self.h, C.c_void_p(jobs.ctypes.data), jobs.size, _dptr(llr), _dptr(payload), _dptr(status),
                                                 _stream_ptr(stream)))

    def uci_polar_decode_list_batch(self, jobs, list_size, llr, payload, status, stream=None):
        """uci_polar_decode_batch with CRC-aided list decoding (list_size 1, 2, 4 or 8) of the fields of 20 bits and more; list size 1
        and the fields of 12..19 bits go through the SSC kernel. Same arguments otherwise. Only enqueues."""
        import torch
        assert isinstance(jobs, np.ndarray) and jobs.dtype == UciPolarJob, "uci_polar_decode_list_batch takes host jobs"
        jobs = np.ascontiguousarray(jobs)
        assert llr.dtype == torch.int8 and payload.dtype == torch.uint8 and status.dtype == torch.uint8
        if jobs.size:  # the extents the kernels may touch lie inside the tensors (the library sees raw pointers)
            assert (jobs["llr_offset"].astype(np.int64) + jobs["nof_llr"].astype(np.int64)).max() <= llr.numel(), "soft bits outside `llr`"
            assert (jobs["payload_offset"].astype(np.int64) + jobs["nof_bits"].astype(np.int64)).max() <= payload.numel(), "payload outside `payload`"
            assert status.numel() >= jobs.size
        check(lib().miphy_uci_polar_decode_list_batch(self.h, C.c_void_p(jobs.ctypes.data), jobs.size, int(list_size), _dptr(llr), _dptr(payload),
                                                      _dptr(status), _stream_ptr(stream)))

    def pucch_process_batch(self, jobs, grid, payload, results, llr=None, stream=None):
        """PUCCH formats 1 and 2 (jobs: numpy PucchJob array, or a uint8 device tensor holding the same bytes): grid complex64 device
        tensor, payload uint8 (one bit per byte), results a uint8 device tensor of n * PucchResult.itemsize bytes (view it with
        .cpu().numpy().view(PucchResult)), llr None or an int8 device tensor for the format-2 soft bits."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, PucchJob)
        assert grid.dtype == torch.complex64 and payload.dtype == torch.uint8 and results.dtype == torch.uint8
        assert results.numel() >= n * PucchResult.itemsize
        assert llr is None or llr.dtype == torch.int8
        check(lib().miphy_pucch_process_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(payload), _dptr(results),
                                              None if llr is None else _dptr(llr), _stream_ptr(stream)))

    def pucch_process_batch_ex(self, jobs, list_size, grid, payload, results, llr=None, stream=None):
        """pucch_process_batch that also takes format-2 PDUs above 11 bits (jobs: numpy PucchJob array, HOST memory only): their soft
        bits are decoded as one polar-coded UCI field each at list size 1, 2, 4 or 8, the payload gets their K bits and the status byte
        of their record the CRC verdict. Other PDUs come out as from pucch_process_batch. Only enqueues."""
        import torch
        assert isinstance(jobs, np.ndarray) and jobs.dtype == PucchJob, "pucch_process_batch_ex takes host jobs"
        jobs = np.ascontiguousarray(jobs)
        assert grid.dtype == torch.complex64 and payload.dtype == torch.uint8 and results.dtype == torch.uint8
        assert results.numel() >= jobs.size * PucchResult.itemsize
        assert llr is None or llr.dtype == torch.int8
        check(lib().miphy_pucch_process_batch_ex(self.h, C.c_void_p(jobs.ctypes.data), jobs.size, int(list_size), _dptr(grid), _dptr(payload),
                                                 _dptr(results), None if llr is None else _dptr(llr), _stream_ptr(stream)))

    def pucch_process_f34_batch(self, jobs, list_size, grid, payload, results, llr=None, est=None, stream=None):
        """PUCCH formats 3 and 4 (jobs: numpy PucchF34Job array, HOST memory only): grid complex64 device tensor, payload uint8 (one bit
        per byte), results a uint8 device tensor of n * PucchResult.itemsize bytes, llr None or an int8 device tensor for the soft bits,
        est None or a float32 device tensor for the estimates the data path used ([port][hop][12 nof_prb] cf_t, then the noise variance
        per port, from each job's est_offset). Payloads above 11 bits are polar decoded at list size 1, 2, 4 or 8. Only enqueues."""
        import torch
        assert isinstance(jobs, np.ndarray) and jobs.dtype == PucchF34Job, "pucch_process_f34_batch takes host jobs"
        jobs = np.ascontiguousarray(jobs)
        assert grid.dtype == torch.complex64 and payload.dtype == torch.uint8 and results.dtype == torch.uint8
        assert results.numel() >= jobs.size * PucchResult.itemsize
        assert llr is None or llr.dtype == torch.int8
        assert est is None or est.dtype == torch.float32
        check(lib().miphy_pucch_process_f34_batch(self.h, C.c_void_p(jobs.ctypes.data), jobs.size, int(list_size), _dptr(grid), _dptr(payload),
                                                  _dptr(results), None if llr is None else _dptr(llr), None if est is None else _dptr(est),
                                                  _stream_ptr(stream)))

    def pucch_process_f0_batch(self, jobs, grid, payload, results, energy=None, jobs_on_device=False, stream=None):
        """PUCCH format 0 (jobs: numpy PucchF0Job array, or with jobs_on_device a uint8 device tensor holding the same bytes, every job with
        a threshold > 0): grid complex64 device tensor, payload uint8 (one bit per byte: nof_harq_ack bytes, then nof_sr), results a uint8
        device tensor of n * PucchResult.itemsize bytes, energy None or a float32 device tensor for the twelve unhopped shift energies of
        each PDU from its energy_offset. Only enqueues."""
        import torch
        assert jobs_on_device == (not isinstance(jobs, np.ndarray)), "host jobs are a numpy array, device jobs a uint8 tensor with jobs_on_device=True"
        jobs, n, ptr, on_dev = self._descs(jobs, PucchF0Job)
        assert grid.dtype == torch.complex64 and payload.dtype == torch.uint8 and results.dtype == torch.uint8
        assert results.numel() >= n * PucchResult.itemsize
        assert energy is None or energy.dtype == torch.float32
        if not on_dev and n:  # the extents the kernel may touch lie inside the tensors (the library sees raw pointers)
            assert (jobs["payload_offset"].astype(np.int64) + jobs["nof_harq_ack"] + jobs["nof_sr"]).max() <= payload.numel(), "payload outside `payload`"
            assert energy is None or jobs["energy_offset"].astype(np.int64).max() + 12 <= energy.numel(), "energies outside `energy`"
        check(lib().miphy_pucch_process_f0_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(payload), _dptr(results),
                                                 None if energy is None else _dptr(energy), _stream_ptr(stream)))

    def srs_pilots_batch(self, jobs, pilots, jobs_on_device=False, stream=None):
        """The transmitted SRS sequences (jobs: numpy SrsJob array, or with jobs_on_device a uint8 device tensor holding the same bytes): pilots a
        complex64 device tensor that receives [symbol][tx port][M] of every job from its pilots_offset. Only enqueues."""
        import torch
        assert jobs_on_device == (not isinstance(jobs, np.ndarray)), "host jobs are a numpy array, device jobs a uint8 tensor with jobs_on_device=True"
        jobs, n, ptr, on_dev = self._descs(jobs, SrsJob)
        assert pilots.dtype == torch.complex64
        if not on_dev and n:  # the extents the kernel may touch lie inside the tensor (the library sees raw pointers)
            size = jobs["nof_symbols"].astype(np.int64) * jobs["nof_tx_ports"] * 12 * jobs["nof_prb"] // np.maximum(jobs["comb_size"], 1)
            assert (jobs["pilots_offset"].astype(np.int64) + size).max() <= pilots.numel(), "sequences outside `pilots`"
        check(lib().miphy_srs_pilots_batch(self.h, ptr, on_dev, n, _dptr(pilots), _stream_ptr(stream)))

    def srs_estimate_batch(self, jobs, grid, h, results, jobs_on_device=False, stream=None):
        """SRS channel estimator (jobs: numpy SrsJob array, or with jobs_on_device a uint8 device tensor holding the same bytes): grid and h
        complex64 device tensors, h receives H[PRG][rx][tx] of every job from its h_offset; results a uint8 device tensor of
        n * SrsResult.itemsize bytes (view it with .cpu().numpy().view(SrsResult)). Only enqueues."""
        import torch
        assert jobs_on_device == (not isinstance(jobs, np.ndarray)), "host jobs are a numpy array, device jobs a uint8 tensor with jobs_on_device=True"
        jobs, n, ptr, on_dev = self._descs(jobs, SrsJob)
        assert grid.dtype == torch.complex64 and h.dtype == torch.complex64 and results.dtype == torch.uint8
        assert results.numel() >= n * SrsResult.itemsize
        if not on_dev and n:  # the extents the kernel may touch lie inside the tensors (the library sees raw pointers)
            i64 = {k: jobs[k].astype(np.int64) for k in ("nof_prb", "prg_size", "nof_rx_ports", "nof_tx_ports", "h_offset", "grid_offset", "grid_nprb")}
            size = i64["nof_prb"] // np.maximum(i64["prg_size"], 1) * i64["nof_rx_ports"] * i64["nof_tx_ports"]
            assert (i64["h_offset"] + size).max() <= h.numel(), "estimates outside `h`"
            assert (i64["grid_offset"] + i64["nof_rx_ports"] * 14 * 12 * i64["grid_nprb"]).max() <= grid.numel(), "grid windows outside `grid`"
        check(lib().miphy_srs_estimate_batch(self.h, ptr, on_dev, n, _dptr(grid), _dptr(h), _dptr(results), _stream_ptr(stream)))

    def precoding_weights_batch(self, jobs, h, weights, metrics=None, jobs_on_device=False, stream=None):
        """Precoding weights from SRS channel matrices (jobs: numpy PrecodingWeightsJob array, or with jobs_on_device a uint8 device tensor holding
        the same bytes): h the complex64 device tensor miphy_srs_estimate_batch wrote, weights a complex64 device tensor that receives
        W[PRG][port][layer] of every UE from its weights_offset (the layout of miphy_precoding), metrics None or a float32 device tensor for
        (lambda, sig, leak) per PRG and layer from each UE's metrics_offset. Only enqueues."""
        import torch
        assert jobs_on_device == (not isinstance(jobs, np.ndarray)), "host jobs are a numpy array, device jobs a uint8 tensor with jobs_on_device=True"
        jobs, n, ptr, on_dev = self._descs(jobs, PrecodingWeightsJob)
        assert h.dtype == torch.complex64 and weights.dtype == torch.complex64 and (metrics is None or metrics.dtype == torch.float32)
        if not on_dev and n:  # the extents the kernels may touch lie inside the tensors (the library sees raw pointers, and the weights' extent)
            for k in range(4):
                used = jobs["nof_ues"] > k
                if not used.any():
                    continue
                u = {f: jobs["ue"][f][used, k].astype(np.int64) for f in PrecodingWeightsUe.names}
                ports, prgs = jobs["nof_ports"][used].astype(np.int64), jobs["nof_prg"][used].astype(np.int64)
                size = u["nof_prb"] // np.maximum(u["prg_size"], 1) * ports * u["nof_ue_ports"]
                assert (u["h_offset"] + size).max() <= h.numel(), "estimates outside `h`"
                assert metrics is None or (u["metrics_offset"] + 3 * prgs * u["nof_layers"]).max() <= metrics.numel(), "metrics outside `metrics`"
        check(lib().miphy_precoding_weights_batch(self.h, ptr, on_dev, n, _dptr(h), _dptr(weights), weights.numel(),
                                                  None if metrics is None else _dptr(metrics), _stream_ptr(stream)))

    def prach_detect_batch(self, jobs, symbols, results, preambles, stream=None):
        """PRACH detector (jobs: numpy PrachJob array, or a uint8 device tensor holding the same bytes), one job per occasion: symbols
        complex64 device tensor, results a uint8 device tensor of n * PrachResult.itemsize bytes, preambles a uint8 device tensor of
        PrachPreambleResult records, one per requested preamble index from each job's preamble_offset (view them with
        .cpu().numpy().view(PrachResult / PrachPreambleResult))."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, PrachJob)
        assert symbols.dtype == torch.complex64 and results.dtype == torch.uint8 and preambles.dtype == torch.uint8
        assert results.numel() >= n * PrachResult.itemsize
        check(lib().miphy_prach_detect_batch(self.h, ptr, on_dev, n, _dptr(symbols), _dptr(results), _dptr(preambles), _stream_ptr(stream)))

    def prach_demodulate_batch(self, sampling_rate_hz, jobs, samples, buffer, stream=None):
        """OFDM PRACH demodulator (jobs: numpy PrachDemodJob array, HOST memory only: one window of one port each): samples and buffer
        complex64 device tensors; a job's rows of L bins go to buffer laid out [td][fd][symbol][L] from its buffer_offset with the
        strides max_nof_fd_occasions and max_nof_symbols, where a PrachJob's symbol_offset can point. Only enqueues."""
        import torch
        assert isinstance(jobs, np.ndarray) and jobs.dtype == PrachDemodJob, "prach_demodulate_batch takes host jobs"
        jobs = np.ascontiguousarray(jobs)
        assert samples.dtype == torch.complex64 and buffer.dtype == torch.complex64
        if jobs.size:  # the extents the kernels may touch lie inside the tensors (the library sees raw pointers)
            i64 = {k: jobs[k].astype(np.int64) for k in ("samples_offset", "nof_samples", "buffer_offset", "nof_td_occasions",
                                                         "max_nof_fd_occasions", "max_nof_symbols")}
            assert (i64["samples_offset"] + i64["nof_samples"]).max() <= samples.numel(), "window outside `samples`"
            rows = i64["nof_td_occasions"] * i64["max_nof_fd_occasions"] * i64["max_nof_symbols"]
            assert (i64["buffer_offset"] + rows * np.where(jobs["format"] < 4, 839, 139)).max() <= buffer.numel(), "PRACH buffer outside `buffer`"
        check(lib().miphy_prach_demodulate_batch(self.h, int(sampling_rate_hz), C.c_void_p(jobs.ctypes.data), jobs.size, _dptr(samples),
                                                 _dptr(buffer), _stream_ptr(stream)))

    def prach_generate_batch(self, jobs, out, stream=None):
        """PRACH frequency-domain preambles y_u,v (jobs: numpy PrachGenJob array or a uint8 device tensor): out complex64 device tensor,
        839 or 139 values per job from its out_offset."""
        import torch
        jobs, n, ptr, on_dev = self._descs(jobs, PrachGenJob)
        assert out.dtype == torch.complex64
        check(lib().miphy_prach_generate_batch(self.h, ptr, on_dev, n, _dptr(out), _stream_ptr(stream)))

    def pdsch_encode_batch(self, tbs, tb_in, codeword_out, stream=None):
        assert isinstance(tbs, np.ndarray) and tbs.dtype == PdschTbDesc
        tbs = np.ascontiguousarray(tbs)
        check(lib().miphy_pdsch_encode_batch(self.h, C.c_void_p(tbs.ctypes.data), tbs.size, _dptr(tb_in), _dptr(codeword_out),
                                             _stream_ptr(stream)))

    def pbch_encode_batch(self, msgs, out, stream=None):
        assert isinstance(msgs, np.ndarray) and msgs.dtype == PbchMsg
        msgs = np.ascontiguousarray(msgs)
        check(lib().miphy_pbch_encode_batch(self.h, C.c_void_p(msgs.ctypes.data), msgs.size, _dptr(out), _stream_ptr(stream)))

    def polar_decode_list_batch(self, code, list_size, crc_mode, n, llr, rnti, msg_out, crc_ok_out, metric_out=None, stream=None):
        check(lib().miphy_polar_decode_list_batch(self.h, C.byref(code), list_size, crc_mode, n, _dptr(llr),
                                                  _dptr(rnti) if rnti is not None else None, _dptr(msg_out), _dptr(crc_ok_out),
                                                  _dptr(metric_out) if metric_out is not None else None, _stream_ptr(stream)))


class PdschProcessPlan:
    """miphy_pdsch_process_plan_*: PDU validation, segmentation and descriptor uploads once; run() is the launches of the transmit chain only."""

    def __init__(self, ctx, pdus):
        assert isinstance(pdus, np.ndarray) and pdus.dtype == PdschPdu
        pdus = np.ascontiguousarray(pdus)
        self.ctx, self.n = ctx, pdus.size
        h = C.c_void_p()
        check(lib().miphy_pdsch_process_plan_create(ctx.h, C.c_void_p(pdus.ctypes.data), pdus.size, C.byref(h)))
        self.h = h

    def run(self, tb_in, grid, stream=None):
        check(lib().miphy_pdsch_process_plan_run(self.h, _dptr(tb_in), _dptr(grid), _stream_ptr(stream)))

    def close(self):
        if getattr(self, "h", None):
            lib().miphy_pdsch_process_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LdpcDecodePlan:
    """miphy_ldpc_decode_plan_*: codeblock descriptors validated, sorted into launch classes and uploaded once; run() is launches only."""

    def __init__(self, ctx, descs):
        assert isinstance(descs, np.ndarray) and descs.dtype == LdpcDecDesc
        descs = np.ascontiguousarray(descs)
        self.ctx, self.n = ctx, descs.size
        h = C.c_void_p()
        check(lib().miphy_ldpc_decode_plan_create(ctx.h, C.c_void_p(descs.ctypes.data), descs.size, C.byref(h)))
        self.h = h

    def run(self, llr, out_bits, iters, stream=None):
        check(lib().miphy_ldpc_decode_plan_run(self.h, _dptr(llr), _dptr(out_bits), _dptr(iters), _stream_ptr(stream)))

    def nof_launches(self):
        return int(lib().miphy_ldpc_decode_plan_nof_launches(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().miphy_ldpc_decode_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PuschDecodePlan:
    """miphy_pusch_decode_plan_*: segmentation and descriptor upload once, run() is launches only."""

    def __init__(self, ctx, tbs):
        assert isinstance(tbs, np.ndarray) and tbs.dtype == PuschTbDesc
        tbs = np.ascontiguousarray(tbs)
        self.ctx, self.n = ctx, tbs.size
        h = C.c_void_p()
        check(lib().miphy_pusch_decode_plan_create(ctx.h, C.c_void_p(tbs.ctypes.data), tbs.size, C.byref(h)))
        self.h = h

    def run(self, llrs, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, stream=None):
        check(lib().miphy_pusch_decode_plan_run(self.h, _dptr(llrs), _dptr(harq_softbits), _dptr(harq_msgs), _dptr(harq_crc_ok), _dptr(tb_out),
                                                _dptr(results), _stream_ptr(stream)))

    def info(self):
        """(codeblocks, dematch-inside-the-decoder flag, largest number of variable nodes)."""
        a = (C.c_uint32 * 3)()
        check(lib().miphy_pusch_decode_plan_info(self.h, a))
        return int(a[0]), bool(a[1]), int(a[2])

    def nof_launches(self):
        """LDPC decoder launches per run (= launch classes of the batch)."""
        return int(lib().miphy_pusch_decode_plan_nof_launches(self.h))

    def enable_timing(self, max_runs=64):
        check(lib().miphy_pusch_decode_plan_enable_timing(self.h, max_runs))

    def read_timing(self):
        """Mean per-kernel milliseconds of the runs since the last call: {"rate_dematch", "ldpc_decode", "tb_assemble", "runs"}."""
        ms, runs = (C.c_float * 3)(), C.c_uint32()
        check(lib().miphy_pusch_decode_plan_read_timing(self.h, ms, C.byref(runs)))
        return {"rate_dematch": float(ms[0]), "ldpc_decode": float(ms[1]), "tb_assemble": float(ms[2]), "runs": int(runs.value)}

    def close(self):
        if getattr(self, "h", None):
            lib().miphy_pusch_decode_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------- HARQ softbuffer pool
class HarqPoolConfig(C.Structure):
    """Mirrors miphy_harq_pool_config (rx_softbuffer_pool_config + the slot period + the extent of one softbuffer)."""
    _fields_ = [("max_softbuffers", C.c_uint32), ("max_nof_codeblocks", C.c_uint32), ("expire_timeout_slots", C.c_uint32),
                ("nof_slots_wrap", C.c_uint32), ("max_codeblocks_per_buffer", C.c_uint32)]


class HarqBufferInfo(C.Structure):
    _fields_ = [("state", C.c_uint32), ("rnti", C.c_uint32), ("harq_id", C.c_uint32), ("nof_codeblocks", C.c_uint32),
                ("first_cb", C.c_uint32), ("expire_slot", C.c_uint32)]


HARQ_AVAILABLE, HARQ_RESERVED, HARQ_LOCKED, HARQ_RELEASED = 0, 1, 2, 3


class HarqPool:
    """miphy_harq_pool: the reference's rx_softbuffer_pool over device-resident HARQ arrays. ctx=None gives a
    bookkeeping-only pool (reservation state machine without device memory; used by the host-logic tests)."""

    def __init__(self, ctx, max_softbuffers, max_nof_codeblocks, expire_timeout_slots, numerology=1, max_codeblocks_per_buffer=0):
        self.cfg = HarqPoolConfig(max_softbuffers, max_nof_codeblocks, expire_timeout_slots, 10240 << numerology, max_codeblocks_per_buffer)
        self.ctx = ctx  # keeps the context alive
        h = C.c_void_p()
        check(lib().miphy_harq_pool_create(ctx.h if ctx is not None else None, C.byref(self.cfg), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().miphy_harq_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, slot, rnti, harq_id, nof_codeblocks):
        """-> (softbuffer index or -1, first codeblock slot = harq_cb_index of the transport-block descriptor)."""
        b, f = C.c_int32(), C.c_uint32()
        check(lib().miphy_harq_pool_reserve(self.h, slot, rnti, harq_id, nof_codeblocks, C.byref(b), C.byref(f)))
        return b.value, f.value

    def lock(self, buffer):
        check(lib().miphy_harq_pool_lock(self.h, buffer))

    def unlock(self, buffer):
        check(lib().miphy_harq_pool_unlock(self.h, buffer))

    def release(self, buffer):
        check(lib().miphy_harq_pool_release(self.h, buffer))

    def run_slot(self, slot):
        check(lib().miphy_harq_pool_run_slot(self.h, slot))

    def info(self, buffer):
        out = HarqBufferInfo()
        check(lib().miphy_harq_pool_info(self.h, buffer, C.byref(out)))
        return out

    def free_codeblocks(self):
        out = C.c_uint32()
        check(lib().miphy_harq_pool_free_codeblocks(self.h, C.byref(out)))
        return out.value

    def arrays(self):
        """Device arrays as torch uint8 / int8 views: (softbits [ncb, 66*384] int8, msgs [ncb, 1056] uint8, crc_ok [ncb] uint8)."""
        import torch
        ptrs = [C.c_void_p() for _ in range(3)]
        check(lib().miphy_harq_pool_arrays(self.h, *[C.byref(p) for p in ptrs]))
        ncb = self.cfg.max_softbuffers * (self.cfg.max_codeblocks_per_buffer or 52)
        dev = torch.device("cuda", self.ctx.device)

        def view(ptr, nbytes, dtype):
            class _Holder:  # __cuda_array_interface__ view over memory the pool owns
                pass
            hld = _Holder()
            hld.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr.value, False), "version": 2}
            t = torch.as_tensor(hld, device=dev)
            return t.view(dtype)
        soft = view(ptrs[0], ncb * HARQ_CB_STRIDE, torch.int8).view(ncb, HARQ_CB_STRIDE)
        msgs = view(ptrs[1], ncb * HARQ_MSG_STRIDE, torch.uint8).view(ncb, HARQ_MSG_STRIDE)
        crc = view(ptrs[2], ncb, torch.uint8)
        return soft, msgs, crc
