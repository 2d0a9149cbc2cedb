"""Build the C part of the oracle (gcc, host only).  TEST INFRASTRUCTURE."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, 'liboracle_vq.so')  # vq_argmin.c + f32_chain.c (the name predates the second source)
SOURCES = ['vq_argmin.c', 'f32_chain.c']


def build(force=False):
    srcs = [os.path.join(HERE, s) for s in SOURCES]
    if force or not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(['gcc', '-O2', '-ffp-contract=off', '-fno-fast-math', '-shared', '-fPIC',
                               *srcs, '-o', SO, '-lm'])
    return SO


if __name__ == '__main__':
    print(build(True))
