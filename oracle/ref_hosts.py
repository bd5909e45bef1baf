"""Builds tests/refhost/ref_dynslam_host.cpp together with the reference's own, unmodified DynSLAM sources
(compiled from where they lie under /root/reference, never copied) into one executable:

  kind "hip"     links dynslam_amd/csrc/libdsr_hip.so (the product);
  kind "oracle"  the same objects compiled with every dsr_* name redirected to the CPU oracle's orc_* by a
                 generated -include header (TEST-ONLY: the checker leg of tests/test_reference_pipeline.py).

Also the reference's driver host (build_driver_host: InfiniTamDriver.cpp + Utils.cpp under shim/host_bench.cpp).

Used by the tests and by __graft_entry__.build_hosts(), which leaves the executables under oracle/_ref/ (OUT): like
oracle/_ref/libref_edges.so they are built where the reference's sources exist and travel with the tree to machines
that do not have them.  Every executable finds its libraries through an $ORIGIN-relative rpath, so that the tree can be
moved after the build,
and run_env() names this tree's library directories in LD_LIBRARY_PATH for wherever OUT itself is put."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/DynSLAM"
HOST = os.path.join(ROOT, "tests", "refhost", "ref_dynslam_host.cpp")
OUT = os.path.join(ROOT, "oracle", "_ref")
DRIVER_HOST = os.path.join(OUT, "ref_driver_host")
PIPELINE_HOST = os.path.join(OUT, "ref_dynslam_host")
PIPELINE_HOST_ORC = os.path.join(OUT, "ref_dynslam_host_orc")
OBJ_DIR = os.path.join(ROOT, "tests", "refhost", "_build")  # object files: stay where they are built
# the reference units of the per-frame pipeline (everything DynSlam::ProcessFrame reaches, GUI excluded)
PIPELINE_UNITS = [
    "DynSlam.cpp", "InfiniTamDriver.cpp", "Utils.cpp", "Input.cpp", "PrecomputedDepthProvider.cpp",
    "InstRecLib/InstanceReconstructor.cpp", "InstRecLib/InstanceTracker.cpp", "InstRecLib/Track.cpp", "InstRecLib/InstanceView.cpp",
    "InstRecLib/InstanceSegmentationResult.cpp", "InstRecLib/SegmentationDataset.cpp", "InstRecLib/SparseSFProvider.cpp",
    "InstRecLib/VisoSparseSFProvider.cpp", "InstRecLib/PrecomputedSegmentationProvider.cpp", "InstRecLib/Utils/BoundingBox.cpp",
    "InstRecLib/Utils/Mask.cpp", "Evaluation/Evaluation.cpp", "Evaluation/CsvWriter.cpp", "Evaluation/Tracklets.cpp",
    "Evaluation/VelodyneIO.cpp", "Evaluation/EvaluationCallback.cpp", "Evaluation/SegmentedCallback.cpp",
    "Evaluation/SegmentedEvaluationCallback.cpp",
]
INC = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "tests", "stubs", "DynSLAM"),
       "-I", os.path.join(ROOT, "tests", "stubs", "DynSLAM", "InstRecLib"),
       "-I", os.path.join(ROOT, "shim", "DynSLAM"), "-I", os.path.join(ROOT, "shim", "DynSLAM", "InstRecLib"),
       "-I", REF, "-I", os.path.join(REF, "InstRecLib")]


def have_reference():
    return os.path.isdir(REF)


def run_env(env=None):
    """Environment to run an executable of OUT with: LD_LIBRARY_PATH starts with this tree's dynslam_amd/csrc and oracle/,
    so that libdsr_hip.so / liboracle.so are found even where OUT does not lie at oracle/_ref/ of this tree (a copy, a link:
    the $ORIGIN-relative rpath then points elsewhere)."""
    env = dict(os.environ if env is None else env)
    dirs = [os.path.join(ROOT, "dynslam_amd", "csrc"), os.path.join(ROOT, "oracle")]
    env["LD_LIBRARY_PATH"] = os.pathsep.join(dirs + [p for p in env.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p])
    return env


def rpath(lib_dir, exe):
    """-Wl,-rpath to lib_dir relative to the directory of exe: valid wherever the tree is checked out or copied to."""
    return "-Wl,-rpath,$ORIGIN/" + os.path.relpath(lib_dir, os.path.dirname(os.path.abspath(exe)))


def inputs():
    return [HOST, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr.h")]


def build(kind, exe, workdir, extra_flags=(), oracle_dir=None):
    """-> exe.  `workdir` receives the object files (and the rename header for kind "oracle").  extra_flags: e.g. sanitizer
    options (compile and link); oracle_dir: where liboracle.so is taken from (a sanitised build for those)."""
    assert kind in ("hip", "oracle")
    os.makedirs(workdir, exist_ok=True)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    flags = ["-std=c++14", "-O1", "-DNDEBUG"] + list(extra_flags)
    if kind == "oracle":
        import sys
        sys.path.insert(0, ROOT)
        from dynslam_amd import _capi
        rename = os.path.join(workdir, "dsr_to_orc.h")
        with open(rename, "w") as f:
            f.write("".join(f"#define dsr_{name} orc_{name}\n" for name in _capi.SIGNATURES))
        flags += ["-include", rename]
        lib_dir = oracle_dir or os.path.join(ROOT, "oracle")
        link = ["-L", lib_dir, "-loracle", rpath(lib_dir, exe), "-fopenmp"] + list(extra_flags)
    else:
        lib_dir = os.path.join(ROOT, "dynslam_amd", "csrc")
        link = ["-L", lib_dir, "-ldsr_hip", rpath(lib_dir, exe), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    jobs = [(os.path.join(REF, u), os.path.join(workdir, u.replace("/", "_") + ".o")) for u in PIPELINE_UNITS]
    jobs.append((HOST, os.path.join(workdir, "ref_dynslam_host.o")))

    def cc(job):
        r = subprocess.run(["g++"] + flags + INC + ["-c", job[0], "-o", job[1]], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{job[0]}:\n{r.stderr[-3000:]}")
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(cc, jobs))
    subprocess.check_call(["g++"] + [o for _, o in jobs] + ["-o", exe, "-lpthread"] + link)
    return exe


def build_driver_host(force=False):
    """-> DRIVER_HOST: shim/host_bench.cpp with -DDSR_HOST_REFERENCE_DRIVER, i.e. the reference's unmodified
    InfiniTamDriver.{h,cpp} + Utils.cpp compiled from where they lie against the shim, linked with libdsr_hip.so."""
    shim = os.path.join(ROOT, "shim")
    src = os.path.join(shim, "host_bench.cpp")
    lib_dir = os.path.join(ROOT, "dynslam_amd", "csrc")
    if force or _stale(DRIVER_HOST, [src, os.path.join(shim, "ITMLib.h"), os.path.join(lib_dir, "libdsr_hip.so")]):
        os.makedirs(OUT, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-DNDEBUG", "-DDSR_HOST_REFERENCE_DRIVER",
                               "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(shim, "DynSLAM"), "-I", REF,
                               src, os.path.join(REF, "InfiniTamDriver.cpp"), os.path.join(REF, "Utils.cpp"), "-o", DRIVER_HOST,
                               "-L", lib_dir, "-ldsr_hip", rpath(lib_dir, DRIVER_HOST), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return DRIVER_HOST


def build_all():
    """The driver host and the reference's whole per-frame pipeline (DynSlam::ProcessFrame and everything it reaches)
    under our test host, once on the HIP library and once on the CPU oracle (the checker of the -m gpu test)."""
    build_driver_host()
    for kind, exe, lib in (("hip", PIPELINE_HOST, os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")),
                           ("oracle", PIPELINE_HOST_ORC, os.path.join(ROOT, "oracle", "liboracle.so"))):
        if _stale(exe, inputs() + [lib, os.path.abspath(__file__)]):
            build(kind, exe, os.path.join(OBJ_DIR, "obj_" + kind))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)
