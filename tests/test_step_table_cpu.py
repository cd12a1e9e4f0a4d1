"""scripts/step_table.py `trace`: the canonical form of a traced plan is a pure function of (items, allocator segments)"""
import ctypes
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _canonical_trace():
    spec = importlib.util.spec_from_file_location('step_table', os.path.join(ROOT, 'scripts', 'step_table.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.canonical_trace


def _plan(*launches):
    """(items, labels) as executor.Plan keeps them; a launch is (entry point, label, args) or (None, label, callback)"""
    items = [(None, a) if ep is None else ((lambda *_: None), a) for ep, _, a in launches]
    labels = [('py' if ep is None else ep, ctx) for ep, ctx, _ in launches]
    return items, labels


SEGMENTS = [(0x7f0000200000, 0x200000), (0x7f0000000000, 0x1000)]      # (unsorted, as an allocator may list them)


def test_pointers_are_named_in_order_of_first_appearance_and_keep_their_sharing():
    a, b = 0x7f0000000010, 0x7f0000200000
    fwd = _plan(('dl3p_f', 'conv_pw:c1', (b, 4, a, b)), ('dl3p_g', 'bn:b1', (a,)))
    bwd = _plan(('dl3p_h', 'conv_pw:c1', (a + 4, b)))
    lines = _canonical_trace()([('fwd',) + fwd, ('bwd',) + bwd], SEGMENTS)
    assert lines == ['fwd dl3p_f conv_pw:c1 p0,4,p1,p0', 'fwd dl3p_g bn:b1 p1', 'bwd dl3p_h conv_pw:c1 p2,p0']


def test_the_last_byte_of_a_segment_is_a_pointer_and_the_next_address_is_not():
    first, size = SEGMENTS[1]
    plan = _plan(('dl3p_f', 'x', (first + size - 1, first + size, first - 1, first)))
    assert _canonical_trace()([('fwd',) + plan], SEGMENTS) == ['fwd dl3p_f x p0,%d,%d,p1' % (first + size, first - 1)]


def test_everything_else_is_written_as_it_is():
    seed = (1234 * 1000003 + 17) | (1 << 62)             # a 63-bit dropout seed: an integer, not an address
    rows = ctypes.c_int(0)
    plan = _plan(('dl3p_f', 'materialize:drop', (None, 0, 0.5, seed, 1.0 / 3.0, ctypes.byref(rows), True, 1 << 20)),
                 (None, 'syncbn:a+b', lambda: None))
    assert _canonical_trace()([('fwd',) + plan], SEGMENTS) == [
        'fwd dl3p_f materialize:drop None,0,0.5,%d,%r,ref,True,1048576' % (seed, 1.0 / 3.0), 'fwd py syncbn:a+b py']


def test_without_segments_no_integer_is_a_pointer():
    plan = _plan(('dl3p_f', 'x', (0x7f0000000010, 3)))
    assert _canonical_trace()([('opt',) + plan], []) == ['opt dl3p_f x %d,3' % 0x7f0000000010]
