"""The seeds of tests/checks/partial_sweep.py that the suite runs: test_gpu_sweeps.py runs them on the device, test_partial_sweep_cpu.py holds
the same draws to the plan functions and to the floors of what they must cover together. A plain module: no test, no fixture."""
PARTIAL_SWEEP_SEEDS = (71, 72, 73, 74)
PARTIAL_SWEEP_N = 15
