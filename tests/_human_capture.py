"""Child process of tests/test_gpu_human_chain.py::test_forward_and_backward_replay_from_one_captured_graph: forward +
backward of ``wire_hip`` captured into one ``torch.cuda.graph`` after a warm-up on a side stream, replayed with a new
pose, expression and triplanes, compared bit for bit with an eager run of the new inputs.  Prints ``RESULT ok``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import human_case as hc      # noqa: E402

DEV = 'cuda:0'


def same(a, b):
    if a.dtype == torch.int64:
        return torch.equal(a, b)
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def main():
    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'ref_human.npz'))
    m = hc.HipHuman(hc.build_case(), DEV)
    changed = hc.POSE_LEAVES + ('expr', 'triplane', 'triplane_face')
    G = hc.cotangents('full', golden['relu/ambiguous_rows'])
    cot = [torch.from_numpy(np.array(G[n])).to(DEV) for n in G]
    leaves = list(m.leaves.values())
    names = list(hc.OUTPUTS) + ['nn_vertex_idxs'] + ['grad ' + k for k in m.leaves]

    def step(capturable):
        assets, refined, offsets = hc.wire_hip(m, True, capturable)
        outs = hc.flat_outputs(assets, refined, offsets)
        return list(outs.values()) + [m.nn_vertex_idxs] + list(torch.autograd.grad([outs[n] for n in G], leaves, cot))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # warm up the allocator outside the capture
        for _ in range(2):
            step(True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(True)
    torch.cuda.synchronize()
    before = [t.clone() for t in static]
    rs = np.random.RandomState(99)
    with torch.no_grad():
        for k in changed:
            new = m.leaves[k].cpu().numpy() * 0.8 + 0.1 * rs.randn(*m.leaves[k].shape)
            m.leaves[k].copy_(torch.from_numpy(new.astype(np.float32)).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static]
    want = step(False)                                   # eager, the index overwrite in place as the reference writes it
    torch.cuda.synchronize()
    differ = [n for n, a, b in zip(names, got, want) if not same(a, b)]
    assert differ == [], 'the replay differs from the eager run in %s' % differ
    # the replay read the new inputs: every output and every leaf gradient moved (the index vector need not)
    stale = [n for n, a, b in zip(names, got, before) if a.dtype != torch.int64 and same(a, b)]
    assert stale == [], 'the replay left %s as captured' % stale
    print('RESULT ok: %d tensors equal the eager run, all of them new' % len(got))


if __name__ == '__main__':
    main()
