"""The sub-wave group walk (csrc/bvq_group_walk.h), what needs no device: the geometry that the edge sweep of
test_gpu_group_walk.py is built on, and the forced-NT build of the library that its NT cases load."""
import ctypes
import os

import pytest

ITEMSIZE = {'f32': 4, 'bf16': 2, 'f16': 2}
# the geometry of the walk, restated: lanes per wave, waves per workgroup, wave loads a wave owns (its window) in the
# forward / encoder / decoder and in the backward
LANES, WAVES, FWD_DEPTH, BWD_DEPTH = 64, 4, 4, 2
NT_BYTES = 256 << 20  # the shipped non-temporal threshold


def lanes_per_group(dn, g):
    return g * ITEMSIZE[dn] // 16


def edge_counts(dn, g):
    """group counts around every boundary of the walk for this L, and one above two workgroups"""
    per_load = LANES // lanes_per_group(dn, g)
    counts = {1}
    for depth in (FWD_DEPTH, BWD_DEPTH):
        for b in (per_load, per_load * depth, per_load * depth * WAVES):   # a load, a window, a workgroup
            counts |= {b - 1, b, b + 1}
    counts.add(2 * per_load * FWD_DEPTH * WAVES + per_load + 1)            # two workgroups, a load and a group
    return sorted(c for c in counts if c >= 1)


def nt0_path():
    from brevitas_amd import _native as nat
    path = os.path.join(os.path.dirname(os.path.abspath(nat.__file__)), 'libbvq_nt0.so')
    assert os.path.exists(path), '%s is not built (python -c "import __graft_entry__ as g; g.build()")' % path
    return path


def test_edge_counts_sit_on_the_boundaries():
    """the sweep's group counts for three values of L, written out"""
    assert edge_counts('bf16', 16) == [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1057]
    assert edge_counts('f32', 256) == [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 34]
    assert edge_counts('f16', 64) == [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 265]


def test_geometry_constants_are_those_of_the_sources():
    """one pair of depths, in the walk's header, and no file of the four families defines a depth of its own"""
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'brevitas_amd', 'csrc')

    def source(f):
        with open(os.path.join(csrc, f)) as fh:
            return fh.read()
    depths = dict(re.findall(r'#define (BVQ_\w+_DEPTH) (\d+)', source('bvq_group_walk.h')))
    assert depths == {'BVQ_GROUP_FWD_DEPTH': str(FWD_DEPTH), 'BVQ_GROUP_BWD_DEPTH': str(BWD_DEPTH)}
    for f in ('bvq_group_quant.hip', 'bvq_group_mse.hip', 'bvq_group_shifted.hip', 'bvq_mx_quant.hip',
              'bvq_group_quant.h'):
        assert not re.search(r'#\s*define\s+\w*DEPTH', source(f)), f


def test_the_forced_nt_variant_keeps_its_threshold_next_to_a_global_libbvq():
    """Both libraries export their internal symbols.  With the package's library in the global scope -- where the C++
    autograd node puts it -- the variant's own calls of bvq::nt_threshold_bytes() must still reach the variant's
    definition; bvq_nt_threshold_bytes() goes through that symbol, so it reports what the entry points compare with."""
    from brevitas_amd import _native as nat
    if os.path.abspath(nat.LIB_PATH) != os.path.join(os.path.dirname(os.path.abspath(nat.__file__)), 'libbvq.so'):
        pytest.skip('BREVITAS_AMD_LIB names another build')
    assert nat.lib.bvq_nt_threshold_bytes() == NT_BYTES
    promoted = ctypes.CDLL(nat.LIB_PATH, mode=ctypes.RTLD_GLOBAL)     # the same handle, now global
    assert promoted.bvq_abi_version() == nat.ABI_VERSION
    variant = nat._load(nt0_path())
    assert variant.bvq_nt_threshold_bytes() == 0
    assert nat.lib.bvq_nt_threshold_bytes() == NT_BYTES
