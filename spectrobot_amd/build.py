"""Build libspectrobot_hip.so for gfx950 with hipcc (in-tree, no JIT cache)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "lib", "libspectrobot_hip.so")
# the translation units: the host API, the coefficient op, the limb family, the state kernel's instances in units by
# (gas counts, slots per block), the instances of five to eight gases, the small operators, the solar source
SOURCES = ["sr_api.hip", "sr_kernels.hip", "sr_limb.hip", "sr_limb_state_12_np8.hip", "sr_limb_state_12_np16.hip",
           "sr_limb_state_34_np8.hip", "sr_limb_state_34_np16.hip", "sr_limb_many.hip", "sr_ops.hip", "sr_solar_source.hip"]
MAX_JOBS = 16  # compiles running at a time
PUBLIC_HEADER = os.path.join(HERE, "..", "include", "spectrobot_hip.h")


def deps():
    """Everything a unit may include: every .hip, .hpp and .inc under csrc/, and the public header."""
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))
            if f.endswith((".hip", ".hpp", ".inc"))] + [PUBLIC_HEADER]


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fno-fast-math", "-fgpu-rdc" if False else "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]


def up_to_date():
    if not os.path.exists(OUT):
        return False
    t = os.path.getmtime(OUT)
    return all(os.path.getmtime(d) <= t for d in deps()) and \
        os.path.getmtime(os.path.abspath(__file__)) <= t


def build(force=False, verbose=False, extra=(), out=None):
    """out: build a variant (extra flags, e.g. -DSR_KTHETA=5) to another path, for
    SPECTROBOT_HIP_LIB=<path>; the default library is never overwritten by a variant."""
    if out is None and extra:
        raise ValueError("a build with extra flags needs its own output path (out=...)")
    if out is None and not force and up_to_date():
        return OUT
    OUT_ = OUT if out is None else os.path.abspath(out)
    return _compile(OUT_, verbose, extra)


def _compile(OUT, verbose, extra):
    """The translation units side by side, at most MAX_JOBS running at a time (the build takes as long as the slowest of
    them: the widest state unit and sr_limb_many.hip are about level, the coefficient op a third of them), then one link;
    objects in a directory of their own beside the library, removed afterwards."""
    from concurrent.futures import ThreadPoolExecutor
    import shutil
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = "%s.tmp.%d" % (OUT, os.getpid())  # other processes never see a half-written library
    objdir = tmp + ".obj"
    os.makedirs(objdir, exist_ok=True)
    objs = [os.path.join(objdir, os.path.splitext(s)[0] + ".o") for s in SOURCES]
    cmds = [[HIPCC] + FLAGS + list(extra) + ["-c", os.path.join(CSRC, s), "-o", o] for s, o in zip(SOURCES, objs)]
    link = [HIPCC] + FLAGS + list(extra) + ["-shared"] + objs + ["-o", tmp]   # (a variant's flags reach the link too)
    if verbose:
        for c in cmds + [link]:
            print(" ".join(c).replace(tmp, OUT))
    try:
        with ThreadPoolExecutor(max_workers=MAX_JOBS) as pool:  # (a thread per running compile: it only waits for it)
            codes = list(pool.map(subprocess.call, cmds))
        for c, rc in zip(cmds, codes):
            if rc:
                raise subprocess.CalledProcessError(rc, c)
        subprocess.check_call(link)
        os.replace(tmp, OUT)
    finally:
        shutil.rmtree(objdir, ignore_errors=True)
        if os.path.exists(tmp):
            os.remove(tmp)
    return OUT


def wait_until_built(timeout=600.0):
    """For the ranks that do not build: wait for the building rank's library."""
    import time
    t0 = time.time()
    while not up_to_date():
        if time.time() - t0 > timeout:
            raise RuntimeError("libspectrobot_hip.so was not built within %.0f s" % timeout)
        time.sleep(0.5)
    return OUT


if __name__ == "__main__":
    # python build.py [--force] [--out PATH -DSR_KTHETA=5 ...]
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    print(build(force="--force" in argv, verbose=True,
                extra=[a for a in argv if a.startswith("-") and a != "--force"], out=out))
