"""The seeds of tests/checks/partial_sweep.py, tests/checks/sampled_sweep.py, tests/checks/widebook_sweep.py and tests/checks/device_view_sweep.py
that the suite runs: test_gpu_sweeps.py runs them on the device, test_partial_sweep_cpu.py / test_sampled_sweep_cpu.py / test_widebook_sweep_cpu.py /
test_device_view_sweep_cpu.py hold the same draws to the plan functions / to the model's premises and to the floors of what they must cover
together. A plain module: no test, no fixture."""
PARTIAL_SWEEP_SEEDS = (71, 72, 73, 74)
PARTIAL_SWEEP_N = 15
SAMPLED_SWEEP_SEEDS = (4, 64, 97, 198)
SAMPLED_SWEEP_N = 4  # drawn cases per seed; the two fixed cases of every seed come on top
WIDEBOOK_SWEEP_SEEDS = (4, 13, 25, 36)
WIDEBOOK_SWEEP_N = 6
DEVICE_VIEW_SWEEP_SEEDS = (23, 24)
DEVICE_VIEW_SWEEP_N = 24
