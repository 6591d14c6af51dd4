"""What the six test_cli_nuclei_* tests of the per-slide point analyses set up in the same way: the checkpoint, the synthetic .npy slide, the
command lines of tools/infer_wsi.py on one and on two ranks, and the run of the tool.  The assertions stay with the tests."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'nuhtc', 'htc_lite_swin_pannuke_infer.py')
TOOL = os.path.join(ROOT, 'tools', 'infer_wsi.py')


def slide_runs(tmp_path, rows_flag):
    """Writes w.pth and the 192 x 320 slide s1.npy into tmp_path -> (base, env, two, folder): the command line up to `rows_flag`
    (--nuclei-feat or --nuclei-graph: the file the rows are compared with), the environment of a run on one rank and on two, and
    folder(run) = <tmp_path>/<run>/nuclei/s1."""
    from nuhtc_amd import synth, weights
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    slide = np.concatenate([np.concatenate(list(synth.nuclei_tiles(5, 64, start=r * 5)), 1) for r in range(3)], 0)    # 192 x 320
    np.save(tmp_path / 's1.npy', slide)
    base = [str(tmp_path / 's1.npy'), CFG, str(ck), '--patch_size', '64', '--step_size', '48', '--batch_size', '8', '--mode', 'qupath', rows_flag]
    env = dict(os.environ, NUHTC_HOST_AFFINITY='0')
    two = dict(env, NUHTC_ONE_DEVICE='1', NUHTC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4')
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        two.pop(key, None)
    return base, env, two, lambda d: tmp_path / d / 'nuclei' / 's1'


def run_tool(cmd, env=None, limit=300):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout
