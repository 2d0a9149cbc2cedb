"""Deterministic mode, host side: the library option and its Python face, the workspace-size queries, and a census of every
atomic add in the kernels.  No GPU: nothing here launches a kernel."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mmvid_amd', 'csrc')


@pytest.fixture()
def lib():
    import mmvid_amd
    from mmvid_amd import _lib
    handle = _lib.load()
    before = mmvid_amd.is_deterministic()
    yield handle
    mmvid_amd.set_deterministic(before)


def get_option(lib, name):
    v = ctypes.c_int(-1)
    assert lib.mmvid_get_option(name.encode(), ctypes.byref(v)) == 0, lib.mmvid_last_error().decode()
    return v.value


# ------------------------------------------------------------------------------------------------- the switch
def test_option_set_and_read_back(lib):
    import mmvid_amd
    assert lib.mmvid_abi_version() == 3
    for flag in (True, False, True):
        prev = mmvid_amd.set_deterministic(flag)
        assert isinstance(prev, bool)
        assert mmvid_amd.is_deterministic() is flag and get_option(lib, 'deterministic') == int(flag)
    assert lib.mmvid_set_option(b'deterministic', 0) == 0 and get_option(lib, 'deterministic') == 0
    assert get_option(lib, 'graphs') == 0  # (the other option is untouched)


def test_context_manager_restores(lib):
    import mmvid_amd
    mmvid_amd.set_deterministic(False)
    with mmvid_amd.deterministic():
        assert mmvid_amd.is_deterministic() and get_option(lib, 'deterministic') == 1
        with mmvid_amd.deterministic(False):
            assert not mmvid_amd.is_deterministic() and get_option(lib, 'deterministic') == 0
        assert mmvid_amd.is_deterministic()
    assert not mmvid_amd.is_deterministic() and get_option(lib, 'deterministic') == 0
    with pytest.raises(ZeroDivisionError):
        with mmvid_amd.deterministic():
            1 / 0
    assert not mmvid_amd.is_deterministic()


@pytest.mark.parametrize('env,want', [(None, False), ('1', True), ('0', False)])
def test_environment_variable_in_a_fresh_process(env, want):
    e = dict(os.environ)
    e.pop('MMVID_DETERMINISTIC', None)
    if env is not None:
        e['MMVID_DETERMINISTIC'] = env
    code = ('import ctypes, mmvid_amd\nfrom mmvid_amd import _lib\nv = ctypes.c_int(-1)\n'
            "assert _lib.load().mmvid_get_option(b'deterministic', ctypes.byref(v)) == 0\n"
            'print(int(mmvid_amd.is_deterministic()), v.value)')
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == [str(int(want))] * 2


def test_unknown_option_names_both(lib):
    assert lib.mmvid_set_option(b'determinstic', 1) != 0
    msg = lib.mmvid_last_error().decode()
    assert "'determinstic'" in msg and 'graphs' in msg and 'deterministic' in msg
    v = ctypes.c_int(0)
    assert lib.mmvid_get_option(b'nope', ctypes.byref(v)) != 0
    assert 'graphs' in lib.mmvid_last_error().decode() and 'deterministic' in lib.mmvid_last_error().decode()


# ------------------------------------------------------------------------------------------------- workspace sizes
def tower_workspace(lib, B, L, layers):
    from mmvid_amd import _lib
    cfg = _lib.TowerCfg(B, L, 768, 12, 3072, layers, 0, -1, 0, -1, 0, 1e-5)
    saved, scratch = ctypes.c_int64(), ctypes.c_int64()
    assert lib.mmvid_tower_workspace(ctypes.byref(cfg), ctypes.byref(saved), ctypes.byref(scratch)) == 0
    return saved.value, scratch.value


# (saved bytes, scratch bytes) that the commit before the deterministic mode reported
TOWER_BYTES_BEFORE = {(6, 579, 12): (1844809728, 315568128), (2, 50, 2): (27182592, 164898304)}


def test_tower_workspace_is_the_same_in_both_modes(lib):
    """Option 0 reports what the library reported before the mode existed.  The mode's slabs live in a region of the scratch arena
    that the backward never used (csrc/tower.hip: det_slab_bytes), so option 1 reports the same bytes: a workspace sized before the
    option was set can never be too small (the GPU test runs a backward that way)."""
    import mmvid_amd
    for (B, L, layers), want in TOWER_BYTES_BEFORE.items():
        mmvid_amd.set_deterministic(False)
        assert tower_workspace(lib, B, L, layers) == want
        mmvid_amd.set_deterministic(True)
        assert tower_workspace(lib, B, L, layers) == want


def test_workspace_queries_grow_with_the_problem(lib):
    q = lib.mmvid_colsum_bf16_det_workspace_bytes
    assert q(1, 768) == 768 * 4 and q(256, 768) == 768 * 4 and q(257, 768) == 2 * 768 * 4
    sizes = [q(m, 768) for m in (1, 100, 256, 257, 3474, 10422)]
    assert sizes == sorted(sizes) and q(3474, 3072) == 4 * q(3474, 768)
    q = lib.mmvid_cross_entropy_fwd_det_workspace_bytes
    assert [q(r) for r in (1, 5, 3474)] == [4, 20, 3474 * 4]
    q = lib.mmvid_attention_bwd_bias_det_workspace_bytes
    assert q(1, 1, 768) == 4 * 3 * 768 * 4 and q(1, 128, 768) == q(1, 1, 768) and q(1, 129, 768) == 2 * q(1, 1, 768)
    assert q(6, 579, 768) == 6 * 5 * 4 * 3 * 768 * 4
    q = lib.mmvid_gemm_bf16_det_workspace_bytes
    assert q(3474, 3072, 1, 0) == 0 and q(3474, 3072, 1, 1) == 55 * 3072 * 4 and q(64, 768, 1, 1) == 768 * 4
    assert q(512, 768, 4, 0) == 4 * 512 * 768 * 4 and q(512, 768, 8, 0) == 2 * q(512, 768, 4, 0)
    q = lib.mmvid_assemble_sequence_bwd_det_workspace_bytes
    rows = (ctypes.c_int64 * 2)(49472, 1025)
    sizes = [q(B, 579, 768, 2, rows) for B in (1, 2, 6, 18)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # the partial chunk sums dominate: at most min(rows, destinations) + rows / 64 + 1 chunks of E floats
    n = 18 * 579
    assert sizes[-1] >= (n + n // 64 + 1) * 768 * 4 and sizes[-1] < (n + n // 64 + 1) * 768 * 4 + (1 << 20)
    assert q(6, 579, 768, 2, (ctypes.c_int64 * 2)(49472, 4096)) >= q(6, 579, 768, 2, rows)
    assert q(6, 579, 768, 1, (ctypes.c_int64 * 1)(1 << 31)) == -1 and q(6, 579, 768, 5, rows) == -1


# ------------------------------------------------------------------------------------------------- census of the atomics
# (file, enclosing function) -> (occurrences of atomicAdd / unsafeAtomicAdd, what makes the training step independent of its order)
DET, EXACT, OFF = 'deterministic counterpart', 'exact (integer)', 'off the training path'
CENSUS = {
    ('attn.hip', 'colsum_rows64'): (1, DET, 'mmvid_attention_bwd_bias_det: template DET stores the wave sums to a slab row'),
    ('embed.hip', 'assemble_fwd_kernel'): (1, EXACT, 'fault counter, unsigned long long'),
    ('embed.hip', 'assemble_bwd_scatter_kernel'): (4, DET, 'mmvid_assemble_sequence_bwd_det'),
    ('embed.hip', 'ce_fwd_kernel'): (2, DET, 'one integer fault counter; the loss term: mmvid_cross_entropy_fwd_det (template DET)'),
    ('embed.hip', 'colsum_bf16_kernel'): (1, DET, 'mmvid_colsum_bf16_det (template DET)'),
    ('embed.hip', 'embdet_keys_kernel'): (1, EXACT, 'int histogram of the inverted index'),
    ('frontend.hip', 'token_rows_gather_kernel'): (1, EXACT, 'fault counter, unsigned long long'),
    ('gemm.hip', 'gemm_epilogue'): (2, DET, 'mmvid_gemm_bf16_det: split-K through slabs, column sums through colsum_det'),
    ('gemm.hip', 'colsum_wave'): (1, DET, 'mmvid_gemm_bf16_det: colsum_det stores to the slab'),
    ('norm.hip', 'ln_bwd_block_sums'): (3, DET, 'the workspace form (mmvid_layernorm_bwd_ws); the mode refuses this branch'),
    ('optim.hip', 'grad_sqnorm_kernel'): (1, DET, 'mmvid_grad_sqnorm_det, the only form the engine calls'),
    ('sample.hip', 'mp_select_keep_kernel'): (2, EXACT, 'int counts of the mask-predict sampler; ' + OFF),
}
_SKIP = {'__launch_bounds__', '__attribute__', 'aligned', 'float', 'int', 'if', 'for', 'while', 'switch', 'defined'}


def scan_text(lines):
    """{enclosing function: occurrences} of one source file.  The enclosing function is the first identifier in front of a '(' on
    the last line that starts in column 0 and is no comment, preprocessor line, closing brace, template / typedef / using line; a
    #define line names its macro.  An atomic in front of any such line is counted under None, which no census entry matches."""
    found, fn = {}, None
    for line in lines:
        code = line.split('//')[0]
        macro = re.match(r'#\s*define\s+(\w+)', code)
        if macro:  # an atomic inside a macro body is counted under the macro's name
            fn = macro.group(1)
        if code[:1] not in ('', ' ', '\t', '}', '#', '\n') and '(' in code and not code.startswith(('template', 'typedef', 'using')):
            names = [m for m in re.findall(r'([A-Za-z_]\w*)\s*\(', code) if m not in _SKIP]
            if names:
                fn = names[0]
        n = len(re.findall(r'\b(?:unsafeAtomicAdd|atomicAdd)\s*\(', code))
        if n:
            found[fn] = found.get(fn, 0) + n
    return found


def scan_atomics():
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith('.hip'):
            for fn, n in scan_text(open(os.path.join(CSRC, name))).items():
                found[(name, fn)] = n
    return found


def test_census_scanner_on_a_synthetic_source():
    """The scanner's heuristic, pinned on the shapes the kernels' sources take: template lines, launch bounds, reference-to-array
    parameters, signatures continued on indented lines, comments that name an atomic, two atomics on one line, a host function."""
    src = '''
// unsafeAtomicAdd(in, a comment) does not count
template <bool DET>
__global__ __launch_bounds__(256) void first_kernel(const float* __restrict__ x,
                                                    float* __restrict__ out) {
    if (DET) out[0] = x[0]; else unsafeAtomicAdd(out, x[0]);  // atomicAdd(in a trailing comment)
}
#define SOMETHING(x) atomicAdd(x, 1)
__device__ __forceinline__ void helper(float (&cs)[32], float* dst) {
    unsafeAtomicAdd(dst, cs[0]), unsafeAtomicAdd(dst + 1, cs[1]);
}
struct S {
    int a;
};
static int host_side(int n) {
    return n;
}
extern "C" int mmvid_entry(float* p, void* stream) {
    hipLaunchKernelGGL(first_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, p, p);
    return 0;
}
__global__ void last_kernel(unsigned long long* c) { atomicAdd(c, 1ull); }
'''
    assert scan_text(src.splitlines(True)) == {'first_kernel': 1, 'SOMETHING': 1, 'helper': 2, 'last_kernel': 1}
    assert scan_text(['    atomicAdd(p, 1);\n']) == {None: 1}  # in front of any function: under None, which the census refuses


def test_census_of_atomic_adds():
    """Every atomicAdd / unsafeAtomicAdd in csrc/*.hip, keyed by file and enclosing function, is accounted for above: it has a
    deterministic counterpart that the mode switches to, or it is an integer sum.  An atomic added to the step without an entry
    (or a second one inside a listed function) fails here."""
    found = scan_atomics()
    want = {k: v[0] for k, v in CENSUS.items()}
    assert found == want, {'unlisted or changed': {k: v for k, v in found.items() if want.get(k) != v},
                           'listed but gone': [k for k in want if k not in found]}
    header = open(os.path.join(ROOT, 'include', 'mmvid_hip.h')).read()
    from mmvid_amd import _lib
    for (f, fn), (_, kind, why) in CENSUS.items():
        assert kind in (DET, EXACT) and why
        if kind == DET:  # the counterpart it names is declared and bound
            sym = re.search(r'mmvid_\w+', why).group(0)
            assert re.search(r'\b' + sym + r'\s*\(', header), sym
            assert sym in _lib.SIGNATURES, sym


def test_new_symbols_are_declared_and_bound(lib):
    from mmvid_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mmvid_hip.h')).read()
    for sym in ('mmvid_get_option', 'mmvid_colsum_bf16_det', 'mmvid_cross_entropy_fwd_det', 'mmvid_assemble_sequence_bwd_det',
                'mmvid_gemm_bf16_det', 'mmvid_attention_bwd_bias_det'):
        assert sym in _lib.SIGNATURES and re.search(r'\b' + sym + r'\s*\(', header) and hasattr(lib, sym)
    for sym in ('mmvid_colsum_bf16_det_workspace_bytes', 'mmvid_cross_entropy_fwd_det_workspace_bytes',
                'mmvid_assemble_sequence_bwd_det_workspace_bytes', 'mmvid_gemm_bf16_det_workspace_bytes',
                'mmvid_attention_bwd_bias_det_workspace_bytes'):
        assert sym in _lib.OTHER and re.search(r'\b' + sym + r'\s*\(', header) and hasattr(lib, sym)
