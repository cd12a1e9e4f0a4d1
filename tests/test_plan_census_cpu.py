"""scripts/plan_census.py: the host-side answers of libdl3p (plans, routes, workspaces, options) as one canonical text file.
No golden file -- the measured tables change with every tuning round -- the census is compared between two builds by hand;
here: the tool runs, is deterministic, and leaves every knob as it found it."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'scripts', 'plan_census.py')


def test_plan_census_runs_twice_alike_and_restores_every_option(tmp_path):
    outs = []
    for name in ('a.txt', 'b.txt'):
        out = tmp_path / name
        r = subprocess.run([sys.executable, TOOL, str(out), '--quick'], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1], 'two runs of the census differ'
    text = outs[0].decode()
    defaults = text.split('\n== ')[0]
    assert defaults.startswith('== defaults\n')
    shape_lines = [l for l in defaults.split('\n') if re.match(r'^\d+ \d+ \d+ q0=', l)]
    assert len(shape_lines) > 100 and all(' q9=' in l and ' ws=' in l and ' wbn=' in l for l in shape_lines)
    dw_lines = [l for l in defaults.split('\n') if l.startswith('dw ')]
    assert dw_lines and all(' q3=' in l and ' wbn=' in l and re.search(r' up=[01]{2} ws=\d+$', l) for l in dw_lines)
    # the geometries of the depthwise edge suite are in: explicit paddings, a residue-class plan (kind 3), a gather (kind 0)
    assert any(' pad=' in l for l in dw_lines) and any(' q0=3,' in l for l in dw_lines) and any(' q0=0,' in l for l in dw_lines)
    got = re.search(r'^get_option (.*)$', defaults, re.M).group(1)
    assert re.fullmatch(r'split_wgrad=-?\d+ conv_sb=-?\d+ sb_rs=-?\d+ sb3=-?\d+ sb_pipe=-?\d+ splitk=-?\d+ no_such_knob=-2147483648', got), got
    # every option the tool moved: accepted, some value of it changes an answer or none does, and after its restore value EVERY
    # line of the census -- the dl3p_get_option line included -- reads as it did before the option was touched
    steps = re.findall(r'^-- option (\w+)=(-?\d+)( \(restore\))? rc(-?\d+): (\d+) lines differ$', defaults, re.M)
    moved = {s[0] for s in steps} - {'no_such_knob'}
    assert len(moved) >= 23, sorted(moved)
    for name, value, restore, rc, differ in steps:
        if name == 'no_such_knob':
            assert int(rc) != 0 and int(differ) == 0
            continue
        assert int(rc) == 0, (name, value, rc)
        if restore:
            assert int(differ) == 0, 'option %s: %s lines differ after its restore value %s' % (name, differ, value)
    assert {s[0] for s in steps if s[2]} == moved, 'an option was moved and not restored'
    # the environment states ran, each in its own process, and at least one of them changes an answer
    envs = re.findall(r'^== (DL3P_\w+=-?\d+): (\d+) lines differ from the defaults$', text, re.M)
    assert len(envs) >= 10 and any(int(n) > 0 for _, n in envs), envs
