# dev (round 6, one GPU call): the new two-rank .svs slide bench test
O=gpurun_out/r06e; mkdir -p $O
timeout 900 python -m pytest tests/test_hip_api.py -m gpu -x -q -k "svs_file_on_every_rank or eight_ranks" 2>&1 | grep -v amdgpu.ids | tail -4 > $O/tests.log; tail -2 $O/tests.log
