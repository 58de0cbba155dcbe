#!/usr/bin/env python3
"""Builds tools/outfile_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and runs it: the output file of the
truth SAM / BAM and of the amplicon, artefact and site support tables (scssim_amd/csrc/scs_outfile.h) as a stand-alone CPU
program -- header, a few buffers and the end-of-file block, plain and BGZF, read back; the error texts of a path that can not be
opened and of a failed write.  Then zlib inflates the BGZF file the program left: it must hold what the plain one holds.  No GPU.

    python tools/outfile_host_check.py [--cxx g++]
"""
import argparse
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "outfile_host_check")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "outfile_host_check.cpp"), "-o", exe])
        rc = subprocess.run([exe, td]).returncode
        if rc == 0:
            plain, z = open(os.path.join(td, "plain.txt"), "rb").read(), open(os.path.join(td, "blocks.gz"), "rb").read()
            if not plain or gzip.decompress(z) != plain or z[-28:] != bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"):
                print("outfile_host_check: the BGZF file does not inflate to the plain one, or lacks the end-of-file block")
                rc = 1
    sys.exit(rc)


if __name__ == "__main__":
    main()
