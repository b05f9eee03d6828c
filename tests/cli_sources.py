"""The sources of the CLI's readers and writers (merkurio_amd/csrc/cli) that a CPU test harness compiles with g++ alone, next to its own
main(): everything that needs neither the library nor a device.  The rest of cli/ (main, commands, the window loops, bgzf_out, tag_host)
calls the library; a harness that wants one of those names it itself and brings its own stubs."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "merkurio_amd/csrc/cli")
_READERS = ("host_mem", "file_bytes", "bgzf_in", "window_source", "fastx", "sam_in", "bam_text", "bam_out", "decompress", "util")


def reader_sources(without=()):
    """-> the .cpp files (all but those named in `without`: a harness that touches a part of the readers only compiles faster),
    then the libraries they need, ready for the end of a g++ line"""
    assert set(without) <= set(_READERS), without
    return [os.path.join(CLI_DIR, name + ".cpp") for name in _READERS if name not in without] + ["-lz", "-ldl", "-lpthread"]
