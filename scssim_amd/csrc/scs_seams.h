// scs_seams.h -- test and tuning seams: environment knobs that change what the library does (small batches, forced kernel
// variants, injected failures, ...).  The PRODUCT library (libscssim_hip.so, bin/scssim) is linked with scs_seams_off.cpp: every
// knob reads as unset and no environment variable of this list is ever looked at.  The tests load libscssim_hip_seams.so
// (SCSSIM_HIP_LIB; bin/scssim_seams) -- the same objects linked with scs_seams_on.cpp, where seam_env is getenv.
//   SCS_TEST_BATCH_SHIFT  pairs per batch = 2^n (many small batches)          SCS_TEST_QK       quality alias rows of 64 / 128 columns
//   SCS_TEST_REDO / _GENERAL / _NO_D1 / SCS_EV_REPLAY  force the read classes' fallbacks     SCS_TEST_SHRINK_OUT  mis-state a batch's text size
//   SCS_READS_SERIAL / SCS_READS_SPLIT / SCS_ERRS_INLINE  launch orders of earlier rounds     SCS_ATTACH_G / SCS_ATTACH_GROUPS  the semi pass as lane groups per template (and how wide)
//   SCS_VMM_FROM_MB / SCS_NO_VMM  where device buffers switch to mapped ranges                SCS_HOST_FASTA / SCS_STAGE_WHOLE  staging paths
//   SCS_TEST_FAIL_AT / SCS_TEST_FAIL_RANK  a CLI rank that dies at a given place
//   SCS_TEST_TRUTH_LDS  bytes of LDS the emit pass of all three truth outputs (SAM, BAM, reference SAM) fills before it copies a run out (small: several runs per workgroup; below a pair: the SAM writes the pair directly, the other two refuse it)
//   SCS_TEST_DEPTH_SLOTS  entries of the depth kernel's LDS table (a power of two up to 512; 4: it overflows into direct adds, 0: no table, every add goes to memory)
//   SCS_TEST_AMP_CHUNK  amplicons per chunk of the amplicon table (scs_amplicons.cpp)       SCS_TEST_AMP_LDS  bytes of its emit pass' LDS run (small: lines straddle two runs)
//   SCS_TEST_SITE_SLAB  genome indices per slab of the artefact table (scs_sites.cpp; small: amplicons and sites on both sides of slab borders; its fill and counting passes also take SCS_TEST_AMP_CHUNK)
//   SCS_TEST_SITE_LDS  bytes of its emit pass' LDS run (small: lines straddle two runs)       SCS_TEST_SITE_PIECE  bytes of its file that cross to the host at a time
//   SCS_TEST_SUPPORT_SLOTS  entries of the site support kernel's LDS table (rounded down to a power of two, at most 1024; 4: it overflows into direct adds, 0: no table)
//   SCS_TEST_LIFT_SLOTS  entries of k_depth_lift's LDS table (depth by reference bin; as SCS_TEST_DEPTH_SLOTS: 4 overflows, 0: no table)
//   SCS_TEST_COV_LDS  buckets of the LDS histogram of the coverage profile's end-of-job pass (at most 4096; 4: most depths overflow into direct adds, 0: no table, every count goes to memory; read at every yield call; the count kernel of the profile on the reference, k_cov_ref_hist, reads it too)
//   SCS_TEST_RUNS_TEXT_CAP  bytes of text a slab of the bedGraph writer holds on the device (scs_runs.cpp; 128 MB unset, at least 1: several slabs in a small job; below one tile's text: the call is refused; read at every write call)
//   SCS_TEST_FASTA_CHUNK  bytes of the raw FASTA per chunk of the device parser, and of a piece of the slice gather (scs_stage.cpp; 64 MB unset, at least 1: chunk borders behind a line end, in a header, between '\r' and '\n', on a '>')
// (SCS_ATTACH_GROUPS / SCS_ATTACH_G began as tuning seams; tests/test_gpu_attach.py now runs k_attach<false, 2 / 4 / 8 / 16> through them.)
#pragma once
namespace scs { const char* seam_env(const char* name); }
