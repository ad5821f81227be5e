"""Test helper: the case lists of tests/test_gpu_lora_wide.py, in a file of their own so that tests/test_lora_wide_host.py can check, without a GPU, that they reach
every instantiation the wide launch functions can select."""
from ucod_dpl_amd import native as N

MAX_N1, MAX_K = N.LORA_WIDE_MAX_N1, N.LORA_WIDE_MAX_K

# (N1, D, r, rows, p_drop): with each N1 every count of column pairs, every r, both row counts and both dropout settings
WIDE_GRAD_CASES = [(8448, 128, 1, 37, 0.0), (8448, 768, 2, 1029, 0.05), (8448, 1280, 8, 37, 0.05), (8448, 1536, 3, 1029, 0.0),
                   (MAX_N1, 128, 8, 1029, 0.05), (MAX_N1, 768, 3, 37, 0.0), (MAX_N1, 1280, 1, 1029, 0.0), (MAX_N1, 1536, 2, 37, 0.05)]
# (rows, K, D): 4224 is the first width past the old limit (16 of the second vector's 512 lanes live); 2053 rows are more than the forward has blocks (2048)
WIDE_FWD_SHAPES = [(111, 4224, 128), (111, 5120, 1280), (2053, MAX_K, 1536)]
# (rows, K, D, live units) for grad_s and both grad_x forms: hidden 4200 pads to 4224; ViT-H+'s 5120
WIDE_OUT_GRAD_SHAPES = [(111, 4224, 128, 4200), (111, 5120, 1280, 5120)]
WIDE_FWD_RANKS = (1, 2, 8)
WIDE_OUT_GRAD_RANKS = (2, 8)
