"""Build libdcsnet_hip.so (the C-ABI library of include/dcsnet_hip.h) for gfx950 with hipcc.

In-tree build: objects under dcs-net_amd/build/, library at dcs-net_amd/lib/libdcsnet_hip.so
(git-ignored, but it travels to the GPU box with the gpurun snapshot).  hipcc cross-compiles
without a GPU.  Usage: python dcs-net_amd/build.py [--force]
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(HERE, 'build')
LIBDIR = os.path.join(HERE, 'lib')
LIB = os.path.join(LIBDIR, 'libdcsnet_hip.so')
ARCH = 'gfx950'
FLAGS = ['-O3', '-std=c++17', '-fPIC', f'--offload-arch={ARCH}', '-Wall', '-Wno-unused-function']
FLAGS += os.environ.get('DCS_EXTRA_HIPCC_FLAGS', '').split()      # diagnostic builds (e.g. -DDCS_PIPE_DIAG)


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith('.hip'))


# Sources that touch ACTIVATIONS are compiled a second time with -DDCS_ACT_BF16 (csrc/dcs_common.h: act_t = bf16 storage,
# entry points suffixed _h): BASELINE configs[4]'s bf16 activations in HBM.
ACT_SOURCES = ('cbn.hip', 'cbn_bwd.hip', 'attention.hip', 'attention_bwd.hip', 'conv_api.hip', 'conv_direct.hip', 'conv_mfma.hip',
               'conv_enc0.hip', 'conv_small.hip', 'conv_wgrad_mfma.hip', 'conv_ring.hip')


def _mfma_source_flags():
    """Every source is compiled WITHOUT the SLP vectoriser, except the two named below: it pairs adjacent scalar fp32 operations
    into v_pk_*_f32, and a packed FMA whose low lane takes the HIGH dword of a source pair (op_sel) loses that lane's
    product beside co-resident bf16-MFMA waves on gfx950 (profiles/r03_pk_fma_op_sel_hazard.txt); packed fp32 VALU beside
    MFMAs is slower than the scalar form anyway (MI355X_MICROARCH.md, cycle constants).  Round 3 did this for the sources that
    issue MFMAs and left 97 VALU kernels carrying such pairs, safe only under stream discipline; since round 4 no kernel of
    the library contains one (same-box A/B of the whole step: profiles/r04_noslp_ab.txt), and tests/test_host_cpu.py scans
    EVERY kernel of the built library for it."""
    # Where the pairing helps and forms no cross-half selection it stays on: the emulated weight-gradient kernel (its g_Y
    # split is packed: +10 % kernel time without) and lstm.hip, whose recurrence kernels (no MFMA) live beside the MFMA
    # A^T B kernel (+40 % on lstm_rec_bwd without) — measured with tools/compare_sequences.py; the ISA test guards both.
    keep_slp = ('conv_wgrad_mfma.hip', 'lstm.hip')
    return {f: ['-fno-slp-vectorize'] for f in _sources() if f not in keep_slp}


def _stamp(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, 'rb') as f:
            h.update(f.read())
    h.update(' '.join(FLAGS).encode())
    return h.hexdigest()


def build(force=False, verbose=True, flags=None, lib=None, objdir=None, per_source_flags=None):
    """Incremental: an object is rebuilt when its source, any header or the flags changed (one stamp per object), the
    library when any object was.  flags / lib / objdir / per_source_flags ({source: [extra flags]}) serve diagnostic
    variants (tools/) — the product build uses the defaults."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = FLAGS if flags is None else flags
    lib = LIB if lib is None else lib
    objdir = OBJ if objdir is None else objdir
    per_source_flags = dict(_mfma_source_flags(), **(per_source_flags or {}))
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    srcs = _sources()
    headers = sorted([os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')] +
                     [os.path.join(HERE, '..', 'include', 'dcsnet_hip.h')])
    hdr_stamp = _stamp(headers)

    def stamp_of(src):
        h = hashlib.sha256()
        with open(os.path.join(CSRC, src), 'rb') as f:
            h.update(f.read())
        h.update(hdr_stamp.encode())
        h.update(' '.join(flags + per_source_flags.get(src, [])).encode())
        return h.hexdigest()

    def compile_one(job):
        src, variant = job
        extra = ['-DDCS_ACT_BF16'] if variant else []
        obj = os.path.join(objdir, src[:-4] + variant + '.o')
        st_file, st = obj + '.stamp', stamp_of(src) + variant
        if not force and os.path.exists(obj) and os.path.exists(st_file) and open(st_file).read() == st:
            return obj, False
        cmd = [hipcc] + flags + per_source_flags.get(src, []) + extra + ['-c', os.path.join(CSRC, src), '-o', obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc failed on {src}:\n{r.stdout}\n{r.stderr}')
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        with open(st_file, 'w') as f:
            f.write(st)
        return obj, True

    jobs = [(s_, '') for s_ in srcs] + [(s_, '_h') for s_ in srcs if s_ in ACT_SOURCES]
    jobs.sort(key=lambda j: -os.path.getsize(os.path.join(CSRC, j[0])))        # the long compiles first
    with ThreadPoolExecutor(max_workers=6) as ex:
        res = list(ex.map(compile_one, jobs))
    objs = [o for o, _ in res]
    stamp_file = os.path.join(objdir, 'stamp.txt')
    stamp = hashlib.sha256(''.join(stamp_of(s_) for s_ in srcs).encode()).hexdigest()
    if (not force and not any(c for _, c in res) and os.path.exists(lib) and os.path.exists(stamp_file) and
            open(stamp_file).read() == stamp):
        return lib
    cmd = [hipcc, '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', lib] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'link failed:\n{r.stdout}\n{r.stderr}')
    with open(stamp_file, 'w') as f:
        f.write(stamp)
    if verbose:
        print(f'built {lib}')
    return lib


if __name__ == '__main__':
    build(force='--force' in sys.argv)
