"""How the CPU tier builds native code: the host libraries of tests/emul/*_emul.cpp, the stand-alone sanitizer programs of
tests/emul/*_san.cpp, and the copied trees with one planted defect each.  A plain module the tests import; it sets nothing in
the environment of this process and preloads nothing.

library() keeps beside every library a record (<library>.dep): its first line is the command that built it, the others are the
files the compiler read (g++ -MMD).  A library is rebuilt when the record is missing, names another command, or names a file
that is newer than the library or gone.  Nothing about a source's includes is written down by hand."""
import concurrent.futures
import glob
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = REPO_ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dusk_zerocaf_amd", "csrc")
EMUL_DIR = os.path.join(HERE, "emul")
ROCM_INC = "/opt/rocm/include"

# -fno-gnu-unique -Wl,-Bsymbolic: a plain and a checked build of the same inline code live in one process, and each must bind its
# own statics (a counter of violated bounds inside an inline function) instead of the first one loaded.
LIBRARY_FLAGS = ("-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-fno-gnu-unique", "-Wl,-Bsymbolic", "-I" + ROCM_INC)
STRICT = ("-Wall", "-Wextra", "-Werror")           # for `flags`: the plan emulations, which include host-only headers
SANITIZE_FLAGS = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
PROGRAM_FLAGS = ("-std=c++17",) + SANITIZE_FLAGS + ("-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INC)
SANITIZER_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def have_rocm():
    return os.path.isdir(ROCM_INC)


def library_name(source, checked=False, sanitize=False):
    """emul.cpp -> libzc_emul.so, ris_dac_emul.cpp -> libzc_ris_dac.so; then _san, then _checked."""
    stem = os.path.splitext(os.path.basename(source))[0]
    if stem.endswith("_emul"):
        stem = stem[:-len("_emul")]
    return "libzc_%s%s%s.so" % (stem, "_san" if sanitize else "", "_checked" if checked else "")


def _fresh(so, command):
    try:
        built = os.path.getmtime(so)
        with open(so + ".dep") as f:
            recorded, *deps = f.read().split("\n")
        return recorded == " ".join(command) and bool(deps) and all(os.path.getmtime(d) <= built for d in deps)
    except OSError:
        return False


def library(source, *, checked=False, sanitize=False, flags=(), root=REPO_ROOT, out_dir=None):
    """Build <root>/tests/emul/<source> for the host -> the library's path, or None without the ROCm headers."""
    if not have_rocm():
        return None
    emul = os.path.join(root, "tests", "emul")
    so = os.path.join(out_dir or emul, library_name(source, checked, sanitize))
    command = ["g++", *LIBRARY_FLAGS, *(SANITIZE_FLAGS if sanitize else ("-O2",)), *(["-DZC_CHECK_BOUNDS"] if checked else []), *flags,
               "-o", so, os.path.join(emul, source)]
    if not _fresh(so, command):
        made = so + ".d"
        if os.path.exists(so + ".dep"):                            # never an old record beside a new library
            os.remove(so + ".dep")
        subprocess.check_call(command + ["-MMD", "-MF", made])
        with open(made) as f:                                      # "target: file file \" lines
            deps = f.read().replace("\\\n", " ").split(":", 1)[1].split()
        os.remove(made)
        with open(so + ".dep", "w") as f:
            f.write("\n".join([" ".join(command)] + [os.path.abspath(d) for d in deps]))
    return so


# ------------------------------------------------------------------ stand-alone sanitizer programs
def sanitizer_program(source, tmp_path, *, checked=False, flags=()):
    """tests/emul/<source> (it has its own main) under AddressSanitizer and UBSan, runtimes linked statically -> the executable's
    path; the calling test is skipped without the ROCm headers.  It runs as a child process; nothing of it is loaded here."""
    if not have_rocm():
        pytest.skip("ROCm headers not present")
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", *PROGRAM_FLAGS, *(["-DZC_CHECK_BOUNDS"] if checked else []), *flags, "-o", exe, os.path.join(EMUL_DIR, source)])
    return exe


def run_vectors(exe, blob, tmp_path, name):
    """Write the blob to tmp_path/name and run the program on it -> the completed process."""
    path = tmp_path / name
    path.write_bytes(bytes(blob))
    return subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, **SANITIZER_ENV), timeout=600)


def assert_clean(run, text):
    assert run.returncode == 0 and text in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-3000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def assert_caught(run, text):
    assert run.returncode == 1 and text in run.stderr, (run.returncode, run.stderr[-500:])


# ------------------------------------------------------------------ planted defects
def _header(entry, headers):
    """The file an entry changes: `headers` is the one file of a catalogue without `header` keys, or maps those keys to files."""
    return headers if isinstance(headers, str) else (headers or {}).get(entry["header"], entry["header"])


def _mutated_copy(where, sources, entry, headers):
    """The layout the emulation sources include through, with the entry's replacement applied to the copied header."""
    csrc = os.path.join(where, "dusk_zerocaf_amd", "csrc")
    emul = os.path.join(where, "tests", "emul")
    os.makedirs(csrc)
    os.makedirs(emul)
    for f in glob.glob(os.path.join(CSRC, "*.h")):
        shutil.copy(f, csrc)
    for s in sources:
        shutil.copy(os.path.join(EMUL_DIR, s), emul)
    if entry is not None:
        path = os.path.join(csrc, _header(entry, headers))
        with open(path) as f:
            text = f.read()
        assert text.count(entry["old"]) == 1, entry["name"]
        with open(path, "w") as f:
            f.write(text.replace(entry["old"], entry["new"]))
    return where


def mutant_builds(tmp_path_factory, catalogue, sources, *, headers=None, needs=None, flags=(), workers=8):
    """One copied tree per entry of the catalogue and one unmutated (key None), each built with library(..., root=copy) on a
    thread pool -> {name: path}, or {name: {key: path}} where `sources` is a {key: source} dict.  `headers`: see _header;
    `needs(entry)` names the keys an entry's verdict loads (default: all).
    The calling fixture is skipped without the ROCm headers.  Nothing is written inside the repository."""
    if not have_rocm():
        pytest.skip("ROCm headers not present")
    several = isinstance(sources, dict)
    by_key = sources if several else {None: sources}
    entries = {None: None, **{m["name"]: m for m in catalogue}}
    jobs = [(name, key) for name, m in entries.items() for key in (by_key if m is None or needs is None else needs(m))]
    dirs = {name: _mutated_copy(str(tmp_path_factory.mktemp(name or "unmutated")), by_key.values(), m, headers) for name, m in entries.items()}
    out = {name: {} for name in entries}
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(workers, 16, os.cpu_count() or 1)) as pool:
        for (name, key), so in zip(jobs, pool.map(lambda j: library(by_key[j[1]], flags=flags, root=dirs[j[0]]), jobs)):
            out[name][key] = so
    assert not any(p.startswith(ROOT + os.sep) for libs in out.values() for p in libs.values())
    return out if several else {name: libs[None] for name, libs in out.items()}


def catalogue_is_sound(catalogue, header_dir=CSRC, headers=None):
    """Names are unique; every `old` occurs exactly once in its header and differs from `new`."""
    names = [m["name"] for m in catalogue]
    assert len(names) == len(set(names))
    for m in catalogue:
        with open(os.path.join(header_dir, _header(m, headers))) as f:
            count = f.read().count(m["old"])
        assert count == 1, "%s: `old` occurs %d times" % (m["name"], count)
        assert m["old"] != m["new"], m["name"]


def assert_killed(entry, failed):
    """The verdict on the labels ("family [case]") a planted defect makes fail."""
    name = entry["name"]
    assert failed != [], "%s survived" % name
    families = {f.split(" [", 1)[0] for f in failed}
    assert set(entry["killers"]) <= families, (name, sorted(families))
    assert not set(entry.get("spared", [])) & families, (name, sorted(families))
    for case in entry.get("cases", []):
        assert case in failed, (name, case, failed[:20])
    for case in entry.get("spared_cases", []):
        assert case not in failed, (name, case)
