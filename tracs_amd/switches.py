"""The environment variables the Python layer reads: one table, one reader.  The library's own are in
csrc/switches.h; tests/test_switches.py holds both tables to the code, to DESIGN.md 8 and to the names the tests set.
Every one is read from the environment at every use."""
import os

# name -> (kind, effect).  Kinds: "flag" set / not set ("=0" is set); "nonempty" set to anything but ""; "text" a word matched at the site
TABLE = {
    "TRACS_DISTANCE_ARRAYS": ("flag", "tracs distance on one GPU: the array route instead of the device-resident one"),
    "TRACS_DIST_PARTITION": ("text", "tracs distance --gpus N: sites (default) or pairs"),
    "TRACS_DIST_PARSE_ALL": ("nonempty", "tracs distance --gpus N: every rank parses the alignment itself instead of receiving the lead's planes"),
    "TRACS_STAGE_TRACE": ("flag", "host entry-point stages on stderr"),
    "TRACS_DIST_BACKEND": ("text", "tracs distance --gpus N: rccl, nccl or gloo (through rccl.backend_choice)"),
    "TRACS_BENCH_BACKEND": ("text", "bench.py's exchange: the same words, read by rccl.backend_choice on its behalf"),
    "TRACS_EXTRA_HIPCC_FLAGS": ("text", "extra flags for tracs_amd/build.py"),
    "HIPCC": ("text", "the compiler tracs_amd/build.py runs (default /opt/rocm/bin/hipcc)"),
    "TRACS_MULTIGPU_WORKER": ("text", "1: this process is a worker that multigpu.launch started (set by it, not by users)"),
}


def get(name, default=None):
    """The value of the switch `name`, or `default` when it is not set.  A name the table does not hold is a KeyError."""
    TABLE[name]
    return os.environ.get(name, default)
