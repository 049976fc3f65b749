"""The cases the tile-w8 tests share: the GPU test runs them, the CPU test asserts from the plan what they reach."""

TOKENS = [17, 31, 33, 97, 129, 257]
# (n_i, r, n_o): one K step; a ragged K step (80 = 64 + 16) and n_o off every tile; four slabs with a ragged last one
# (1040 = 3 x 320 + 80, itself 64 + 16); five K steps, the last ragged, S = 1
SHAPES = [(64, 16, 24), (80, 48, 520), (1040, 16, 136), (272, 64, 72)]
