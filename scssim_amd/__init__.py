"""scssim_amd -- host-side mirror of the SCSsim `genreads` interface over the MI355X C ABI.

The product is `libscssim_hip.so` (hand-written gfx950 kernels + C ABI, include/scssim_hip.h) and the
`scssim` CLI.  This package is ctypes plumbing for tests, bench.py and torch.distributed drivers:
method names follow the reference's call sequence (src/scssim.cpp:46-67: loadData, train(profile),
createFrags, amplify, yieldReads).  There is no CPU fallback: importing works anywhere, creating a
`GenReads` needs the built library and a GPU, and fails loudly otherwise.
"""
from .api import (GenReads, ScsError, Profile, fasta_probe, fasta_write_index, lib_path, load_library, build,  # noqa: F401
                  merge_fastq_shards, merge_fastq_parts, part_paths, text_checksum, gpu_local_cpus, bgzf_probe, batch_plan_probe, bgzf_blocks, bgzf_device_probe, scan_probe, alloc_plan_probe, alloc_sums_probe, ALLOC_SLOTS, ALLOC_CHUNK, comm_unique_id, simuvars_probe, devbuf_probe, truth_record_probe, truth_bam_record_probe, live_resources, depth_layout_probe, depth_read_probe, coverage_read_probe, coverage_stats_probe, coverage_tile, coverage_finish_probe, gc_bias_probe, coverage_ref_finish_probe, runs_probe, runs_line_probe, amplicon_line_probe, artefact_probe, artefact_ref_probe, support_read_probe, support_ref_probe, support_ref_header_probe, site_support_line_probe, LiftTable, lift_plan_probe, lift_file_probe, lift_read_probe, truth_ref_record_probe,
                  SCS_OK, SCS_EINVAL, SCS_EIO, SCS_EDEVICE, SCS_EOVERFLOW)
