"""The six-value hopping-parameter scan on the sample operator that tests/test_gpu_kscan.py runs as one batched solve: the
values, the solver parameters and the step at which the CPU oracle, in the reference's summation order, stops each of them
(tests/test_kscan_cases.py checks those on the CPU).  Five distinct stopping steps and one column that never stops."""
SCAN_KS = [0.05, 0.10, 0.15, 0.15 + 0.05j, 0.18, 0.20]
SCAN_RESTART, SCAN_MAX_ITER, SCAN_TOL = 5, 400, 1e-10
SCAN_RHS_SEED = 1                      # problems.rhs_grid(3072, 1), the same in every column
SCAN_STOPS = [32, 43, 88, 104, 360, 400]   # 400 = max_iter: k = 0.20 does not converge
