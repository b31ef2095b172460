"""How csrc/Makefile builds the units of libsvbrdf_hip.so (a .hip file each, one pattern rule), for the CPU tests of those
units -- the only place in tests/ that asks make for its variables and compiles a unit: the Makefile's variables, a unit's
device assembly with exactly its flags, a unit alone as a library of its own, the commands `make` would run, and the two
statements every unit's test makes about the layout -- the Makefile builds the unit into the library, and what units
share lives in headers that hold no kernel and no entry point."""
import os
import re
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svbrdf_estimation_amd", "csrc")


def make_var(name):
    """the words of a Makefile variable (`make print-NAME`)"""
    return subprocess.check_output(["make", "-s", "-C", CSRC, "print-" + name], text=True).strip().split()


def _compile(unit, sched_var, extra, how, out):
    """<unit>.hip -- or the path of a source that includes one -- with HIPCC, HIPFLAGS, the scheduler set `sched_var`
    names (None: none, as the Makefile gives the unit none) and `extra` (-D...), `how` into `out`"""
    source = unit if os.path.isabs(unit) else os.path.join(CSRC, unit + ".hip")
    cmd = make_var("HIPCC") + make_var("HIPFLAGS") + (make_var(sched_var) if sched_var else []) + list(extra)
    cmd += how + ["-o", out, source]
    cmd = [c.replace("../../include", os.path.join(ROOT, "include")) for c in cmd]
    subprocess.check_call(cmd, cwd=CSRC, stderr=subprocess.DEVNULL)


def compile_unit_asm(tmp, unit, sched_var=None, extra=()):
    """Device-only assembly of a unit -- its name ("svbrdf_photo_fit"), or the path of a source that includes one -- with
    exactly the Makefile's flags for it, and `extra`."""
    out = str(tmp / (os.path.splitext(os.path.basename(unit))[0] + ".s"))
    _compile(unit, sched_var, extra, ["-S", "--cuda-device-only"], out)
    with open(out) as f:
        return f.read()


def dot3_probe_instructions(tmp, unit, sched_var=None):
    """The numerics contract on the coords -> NH path, in a unit's own build: a kernel that is dot3 (svbrdf_device.h) and
    nothing else, compiled behind the unit's source with the unit's flags.  -> (the mnemonics of its vector instructions
    other than moves, its FMA count); the contract is 3 v_mul_f32 + 2 v_add_f32 and no FMA."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    src = tmp / "probe.hip"
    src.write_text('#include "%s"\n'
                   'extern "C" __global__ void svbrdf_isa_probe_dot3(const float *__restrict__ a, float *__restrict__ o)\n'
                   '{\n'
                   '    o[threadIdx.x] = dot3(a[threadIdx.x], a[threadIdx.x + 64], a[threadIdx.x + 128], a[threadIdx.x + 192],\n'
                   '                          a[threadIdx.x + 256], a[threadIdx.x + 320]);\n'
                   '}\n' % os.path.join(CSRC, unit + ".hip"))
    _, _, whole, _, ins, _ = isa_stats.analyse(compile_unit_asm(tmp, str(src), sched_var), "svbrdf_isa_probe_dot3")
    return [mn for _, _, mn, _ in ins if mn and mn.startswith("v_") and not mn.startswith("v_mov")], whole["fma"]


def build_unit_library(tmp, unit, sched_var=None, extra=()):
    """The unit alone, the Makefile's flags for it and `extra`, linked into a .so of its own under `tmp` (enough for what
    reads a library's offload bundle, not for loading it).  -> the library's path"""
    os.makedirs(str(tmp), exist_ok=True)
    obj, so = str(tmp / (unit + ".o")), str(tmp / ("lib" + unit + ".so"))
    _compile(unit, sched_var, extra, ["-c"], obj)
    subprocess.check_call(make_var("HIPCC") + ["--offload-arch=gfx950", "-fPIC", "-shared", "-o", so, obj], stderr=subprocess.DEVNULL)
    return so


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
    """The unit (or the header `unit` names in full) includes the header, and the header shares device functions and host
    helpers only: no kernel, no entry point.  -> the header's text"""
    includer = unit if unit.endswith(".h") else unit + ".hip"
    assert header.endswith(".h") and '#include "%s"' % header in read_csrc(includer), (unit, header)
    text = read_csrc(header)
    assert "__global__" not in text and 'extern "C" {' not in text, header
    return text
