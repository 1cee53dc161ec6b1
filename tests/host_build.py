"""TEST INFRASTRUCTURE ONLY -- builds and runs the stand-alone host programs of tests/harness/ for the CPU tests: a shared library that
ctypes loads, or the sanitized program (its own main) that runs as a child process.  A sanitizer runtime never enters a Python process."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, 'tests', 'harness')
OUT = os.path.join(HARNESS, '_build')
SANITIZE = ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']


def compile(source_name, out_name, flags):
    """g++ tests/harness/<source_name> -> tests/harness/_build/<out_name>; returns the path."""
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, out_name)
    r = subprocess.run(['g++', '-O2', '-std=c++17'] + list(flags) + ['-o', out, os.path.join(HARNESS, source_name)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return out


def shared_lib(source_name, long_returning=()):
    """dsdf_x_host.cpp -> libdsdf_x_host.so, loaded; the functions named in `long_returning` return a C long."""
    stem = os.path.splitext(source_name)[0]
    lib = C.CDLL(compile(source_name, f'lib{stem}.so', ['-shared', '-fPIC']))
    for name in long_returning:
        getattr(lib, name).restype = C.c_long
    return lib


def sanitized_program(source_name):
    """dsdf_x_host.cpp -> the program dsdf_x_host_asan, built with AddressSanitizer + UBSan; returns its path."""
    return compile(source_name, os.path.splitext(source_name)[0] + '_asan', SANITIZE)


def run_case(exe, path, verdict=' 0 mismatches'):
    """Runs the stand-alone program on one case file: it ends with status 0, reports `verdict`, and no sanitizer spoke."""
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, (str(path), r.stdout)
    assert verdict in r.stdout and 'runtime error' not in r.stdout and 'AddressSanitizer' not in r.stdout, (str(path), r.stdout)


def ptr(a):
    """The data pointer of a numpy array for a ctypes call; None stays None (a null pointer)."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
