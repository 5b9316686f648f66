"""Build libfaststyle_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

Every .hip source is compiled to its own object under faststyle_amd/build/ (in parallel, re-used
while neither the source nor any header changed), then linked into the shared library."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["fs_conv.hip", "fs_wino.hip", "fs_wino2.hip", "fs_wino2h.hip", "fs_wino4.hip", "fs_wino4t.hip", "fs_wino4t1b.hip", "fs_wino4t1c.hip", "fs_wino4t1d.hip", "fs_wino4t4a.hip", "fs_wino4t4b.hip", "fs_wino4t2.hip", "fs_wino4t2b.hip", "fs_wino6.hip", "fs_wgrad.hip", "fs_wgrad2.hip", "fs_wgw.hip", "fs_elem.hip", "fs_fold.hip", "fs_io.hip", "fs_feed.hip", "fs_jpeg.hip", "fs_jpegenc.hip", "fs_cvresize.hip", "fs_yuv.hip", "fs_yuv16.hip", "fs_compose.hip", "fs_mix.hip", "fs_temporal.hip", "fs_resample.hip", "fs_guided.hip", "fs_tnet.hip", "fs_bf16.hip", "fs_bstream.hip", "fs_vgg.hip", "fs_c3.hip", "fs_cstream.hip", "fs_s16.hip", "fs_gram.hip", "fs_api.hip"]
OUT = os.path.join(HERE, "libfaststyle_hip.so")
OBJDIR = os.path.join(HERE, "build")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-pass-failed"]
# No SLP vectorisation anywhere (round 5; round 4 had it off in the F(4x4) files only).  With it (ROCm 7.2 clang) two of the three epilogue
# instantiations of fs_wino4.hip return WRONG values on gfx950 (a few per cent of the elements, always lanes 12-15 of a row of 16 and the odd
# channel of a pair; tools/w4_slp_repro.py on the GPU with an -fslp-vectorize build) while the CPU emulator build of the same source is right and
# the third instantiation, equally packed, is right too.  The cause was not isolated (no undefined behaviour left in the source; a code-generation
# or hazard problem around v_pk_add_f32 / v_pk_fma_f32 -- see FS_W4_MFMA_SETTLE in csrc/fs_wino4.h for the hazard the compiler cannot see).
# Packed fp32 beside fp32 matrix instructions is slower anyway (MI355X_MICROARCH.md: price of one filler beside MFMAs), the kernels that want a
# packed instruction write it as inline assembly (fs_kernels.h: fs_pk_add / fs_wino_cols01), and the parity suite is the only guard against a
# silently wrong vectorisation in the other twenty translation units: they are compiled without it unless listed in FILE_FLAGS below.  Measured
# (DESIGN.md section 10): no change of any bench leg except through fs_wgw.hip, which is therefore allow-listed.
FLAGS.append("-fno-slp-vectorize")
# The allow-list: translation units that are compiled WITH the vectoriser because it was measured to pay and their GPU parity tests cover the
# vectorised code.  fs_wgw.hip (Winograd filter gradients): its commit phase is straight float4 arithmetic on loaded tiles (affine + ReLU, the
# B^T x B and G dz G^T transforms) that the vectoriser packs; without it wgw_kernel is 3.4 % slower (1.060 against 1.025 ms per batch-32 step, same
# lease, two alternations: step 17.68 against 17.61 ms).  Its matrix instructions are compiler builtins (no inline-assembly accumulators), round 4
# shipped it vectorised, and tests/test_kernels_parity.py::test_winograd_filter_gradient_matches_oracle[hip-*] plus every path-level gradient test
# run through it on the GPU.
FILE_FLAGS = {"fs_wgw.hip": ["-fslp-vectorize"]}
# The allow-list holds for the compiler it was validated with (the GPU parity suite ran against THIS clang's vectorised fs_wgw.hip): any other
# hipcc -- a ROCm bump -- builds every translation unit without the vectoriser (the safe configuration; costs 0.4 % of a batch-32 step) until
# the GPU suite has been run with it and this string updated.  FS_BUILD_SLP_ALLOWLIST=1 / 0 overrides the check.
VALIDATED_CLANG = "roc-7.2.0 26014 7b800a19466229b8479a78de19143dc33c3ab9b5"


def allowlist_active(hipcc):
    force = os.environ.get("FS_BUILD_SLP_ALLOWLIST")
    if force in ("0", "1"):
        return force == "1"
    try:
        v = subprocess.run([hipcc, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode(errors="replace")
    except OSError:
        return False
    return VALIDATED_CLANG in v

def source_digest():
    """sha256[:16] over the kernel sources (csrc/*.hip, csrc/*.h, the public headers): the identity of the build a stored measurement
    (profiles/*hbm_traffic*.json) belongs to -- there is no .git on the GPU box, so a commit id is not available where profiles are collected."""
    import hashlib
    h = hashlib.sha256()
    inc = os.path.join(os.path.dirname(HERE), "include")
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))) + \
        sorted(os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def build(force=False, verbose=False, extra_flags=(), out=None, objdir=None, file_flags=None):
    """extra_flags: appended for every source (a later -f flag wins); file_flags: {source name: [flags]} appended for single sources
    (experiments: e.g. the round-4 configuration is extra_flags=['-fslp-vectorize'], file_flags={f: ['-fno-slp-vectorize'] for the fs_wino4* files})."""
    out = out or OUT
    objdir = objdir or OBJDIR
    file_flags = FILE_FLAGS if file_flags is None else file_flags
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    headers = [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")] + \
        [os.path.join(os.path.dirname(HERE), "include", h) for h in ("faststyle_hip.h", "faststyle_io.h")]
    hdr_time = _newest(headers + [os.path.abspath(__file__)])
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if file_flags is FILE_FLAGS and file_flags and not allowlist_active(hipcc):
        if verbose:
            print("faststyle build: hipcc is not the compiler the SLP allow-list was validated with -- building every file with -fno-slp-vectorize", flush=True)
        file_flags = {}
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    objs = []
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s) + ".o")
        objs.append(o)
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(s), hdr_time):
            jobs.append([hipcc] + FLAGS + list(extra_flags) + file_flags.get(os.path.basename(s), []) + ["-I", CSRC, "-c", s, "-o", o])
    if not jobs and os.path.exists(out) and os.path.getmtime(out) >= _newest(objs):
        return out

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return r.returncode, r.stdout.decode(errors="replace"), cmd

    with ThreadPoolExecutor(max_workers=min(len(jobs) or 1, os.cpu_count() or 4)) as ex:
        for rc, log, cmd in ex.map(run, jobs):
            if log.strip():
                sys.stderr.write(log)
            if rc != 0:
                raise subprocess.CalledProcessError(rc, cmd)
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out]
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.check_call(link)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
