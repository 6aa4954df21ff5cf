"""Building and reading for the CPU-side tests: the tests/host_check/*_check.cpp libraries, the tests/c/*.c programs, the public
header's text and a library's exported names.
tests/host_check/: policy_check.cpp -> test_policy_lane_on_host.py; cofactor_check.cpp -> test_cofactor_lane_on_host.py;
dom2_check.cpp -> test_dom2_on_host.py; digest_check.cpp -> test_digest_lane_on_host.py; keyed_check.cpp -> test_keyed_on_host.py;
keyed_comb_check.cpp -> test_keyed_comb_on_host.py; keyed_forms_check.cpp -> test_keyed_forms_on_host.py; keyed_rlc_check.cpp ->
test_keyed_rlc_on_host.py; signer_check.cpp -> test_sign_keyed_on_host.py; crafted_check.cpp -> test_crafted_scalars_on_host.py;
host_check.cpp -> conftest.py's `hostcheck`."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libeddsa_amd")
ROCM = "/opt/rocm"

# (conftest.py's `hostcheck` fixture builds host_check.cpp with its own copy of these flags)
CHECK_FLAGS = ["-std=c++17", "-O2", "-fPIC", "-shared", "-DED_HOST_CHECK", "-Wno-unknown-pragmas",
               "-I" + os.path.join(LIBDIR, "csrc")]


def build_check(tmp_path_factory, name):
    """tests/host_check/<name>_check.cpp - device source compiled for the host CPU - as a ctypes.CDLL in a temporary directory"""
    lib = str(tmp_path_factory.mktemp(name + "check") / ("lib" + name + "check.so"))
    subprocess.check_call(["g++", *CHECK_FLAGS, os.path.join(ROOT, "tests", "host_check", name + "_check.cpp"), "-o", lib])
    return ctypes.CDLL(lib)


def c_program_command(exe, source, *, libs, wall=False, threads=False, rocm=False):
    """the command line that builds tests/c/<source> against the library libs[0] of libeddsa_amd/ (found at run time through an
    rpath), then libs[1:]; rocm: the program calls HIP itself"""
    return (["gcc", "-std=c11", "-O1"] + ["-Wall"] * wall + ["-pthread"] * threads
            + ["-I" + os.path.join(ROOT, "include")] + ["-I" + ROCM + "/include"] * rocm
            + [os.path.join(ROOT, "tests", "c", source), "-L" + LIBDIR, "-l" + libs[0]]
            + ["-L" + ROCM + "/lib", "-lamdhip64"] * rocm
            + ["-Wl,-rpath," + LIBDIR] + ["-Wl,-rpath," + ROCM + "/lib"] * rocm
            + ["-l" + name for name in libs[1:]] + ["-o", str(exe)])


def build_c_program(tmp_path, source, **how):
    """-> the path of the program built from tests/c/<source> in tmp_path (see c_program_command)"""
    exe = tmp_path / os.path.splitext(source)[0]
    subprocess.check_call(c_program_command(exe, source, **how))
    return exe


def header_text(strip_comments=False, name="eddsa_amd.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip_comments else text


def declared_names(text, macro):
    """the functions a header's text declares behind `macro`, which is a regular expression: r"RFC8032_EDDSA_DECL", or
    r"(?<![0-9A-Z_])EDDSA_AMD_DECL" where the longer macro names that end in the same letters must not count"""
    return set(re.findall(macro + r"\s+[\w\s\*]+?\b(\w+)\s*\(", text))


def exported_names(lib_path):
    """the functions a shared library defines and exports; a bare file name is looked up in libeddsa_amd/"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib_path)], text=True)
    return {l.split()[-1] for l in out.splitlines() if " T " in l}       # (kernel handles and __hip_cuid_* are data symbols)
