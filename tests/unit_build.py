"""How csrc/Makefile builds the single-source units of libsvbrdf_hip.so (svbrdf_aux_f64, svbrdf_photo_*, svbrdf_capture),
for the CPU tests of those units: the Makefile's variables, a unit's device assembly with exactly its flags, the commands
`make` would run, and the two statements every unit's test makes about the layout -- the Makefile builds the unit into
the library, and what units share lives in headers that hold no kernel and no entry point.  (The K3 guards compile
svbrdf_kernels.hip, which has rules of its own: tests/test_isa_guard.py.)"""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svbrdf_estimation_amd", "csrc")


def make_var(name):
    """the words of a Makefile variable (`make print-NAME`)"""
    return subprocess.check_output(["make", "-s", "-C", CSRC, "print-" + name], text=True).strip().split()


def compile_unit_asm(tmp, unit, sched_var=None):
    """Device-only assembly of a unit -- its name ("svbrdf_photo_fit"), or the path of a source that includes one -- with
    HIPCC, HIPFLAGS and the scheduler set `sched_var` names (None: none, as the Makefile gives the unit none)."""
    source = unit if os.path.isabs(unit) else os.path.join(CSRC, unit + ".hip")
    out = str(tmp / (os.path.splitext(os.path.basename(source))[0] + ".s"))
    cmd = make_var("HIPCC") + make_var("HIPFLAGS") + (make_var(sched_var) if sched_var else [])
    cmd += ["-S", "--cuda-device-only", "-o", out, source]
    cmd = [c.replace("../../include", os.path.join(ROOT, "include")) for c in cmd]
    subprocess.check_call(cmd, cwd=CSRC, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def make_commands():
    """the commands a full build runs (`make -n -B`), each as its list of words"""
    text = subprocess.check_output(["make", "-n", "-B", "-C", CSRC], text=True)
    return [shlex.split(line) for line in text.splitlines() if line.strip() and not re.match(r"make(\[\d+\])?:", line)]


def read_csrc(*names):
    """the text of the named files of csrc/, joined: a unit and the headers it owns"""
    text = []
    for name in names:
        with open(os.path.join(CSRC, name)) as f:
            text.append(f.read())
    return "\n".join(text)


def assert_makefile_builds(unit, sched_var=None):
    """Exactly one command of a full build compiles <unit>.hip; it holds every word of HIPFLAGS and the unit's scheduler
    set, in the set's order (without one: no -mllvm option at all); the link command lists the unit's object."""
    commands = make_commands()
    compiles = [c for c in commands if "-c" in c and os.path.basename(c[-1]) == unit + ".hip"]
    assert len(compiles) == 1, (unit, compiles)
    cmd = compiles[0]
    flags = make_var("HIPFLAGS")
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags, flags
    assert all(w in cmd for w in flags), (unit, [w for w in flags if w not in cmd])
    if sched_var:
        sched = make_var(sched_var)
        assert sched and any(cmd[i:i + len(sched)] == sched for i in range(len(cmd))), (unit, sched, cmd)
    assert cmd.count("-mllvm") == (make_var(sched_var).count("-mllvm") if sched_var else 0), (unit, cmd)
    obj = cmd[cmd.index("-o") + 1]
    assert os.path.basename(obj) == unit + ".o", obj
    links = [c for c in commands if "-shared" in c]
    assert len(links) == 1 and obj in links[0] and os.path.basename(links[0][links[0].index("-o") + 1]) == "libsvbrdf_hip.so", links


def assert_includes_shared_header(unit, header):
    """The unit includes the header, and the header shares device functions and host helpers only: no kernel, no entry
    point.  -> the header's text"""
    assert header.endswith(".h") and '#include "%s"' % header in read_csrc(unit + ".hip"), (unit, header)
    text = read_csrc(header)
    assert "__global__" not in text and 'extern "C" {' not in text, header
    return text
