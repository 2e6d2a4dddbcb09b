"""One float64 case per persistent recurrence instance the launch dispatch can select (lstm.hip, lstm5.hip).

For each layer the host picks ONE template instance of a kernel family from H, D, the cell, the precision mode, T * B * D * 4H * 4
(the v5 stash limit) and the batch (through make_plan3 / make_plan2: the group count G, then the rows per group Bg, then BQ = 1 / 2 / 4
row quads).  ROWS names, for every instance the dispatch reaches on a 256-CU MI355X, one shape and the forward and backward instance
it must launch.  Each row runs forward + backward of one layer through the module with ragged lengths (one full row, one 1-frame row,
a partial last group), asserts from the launch record (rnnt_hip_lstm_launch_log) that exactly the declared instances ran, and checks
against torch float64: fp32 rows with the bounds of test_gpu_lstm.py, fp16 rows with those of test_gpu_f16_compute.py.

test_every_compiled_instance_is_declared_or_unreachable (no GPU) lists the recurrence kernels compiled into librnnt_hip.so: each is
declared by a row or named in UNREACHABLE, and each declared instance exists, so a dispatch change that adds an instance fails here
until a row tests it.
"""
import re
import struct

import pytest
import torch
import torch.nn as nn

from tests.test_gpu_f16_compute import GRAD_COS, GRAD_RNORM, OUT_ATOL, _grad_stats
from tests.test_gpu_lstm import FWD_ATOL, GRAD_RTOL, _poison_free_memory

# Instance names: kernel without "_kernel", every template argument in order (defaults included), bools as 0 / 1
# (ops.recurrence_instance).  The cell argument C is 0 LSTM, 1 GRU, 2 Elman (tanh and ReLU share it); the last argument of the v5
# kernels is the one-product (fp16) form.  Columns: forward instance, backward instance, cell, B, T, I, H, D, precision, env switch.
ROWS = [
    # v1 (lstm.hip, LSTM only): 4- / 8-unit slices (MT = 1 / 2) x 16 / 32 / 64 padded rows (NT = 1 / 2 / 4), MT * NT <= 4;
    # RNNT_LSTM_V1 forces them
    ('lstm_fwd<1,1>',         'lstm_bwd<1,1>',               'lstm',     13,  6, 12,   16, 2, 'fp32', 'RNNT_LSTM_V1'),
    ('lstm_fwd<1,2>',         'lstm_bwd<1,2>',               'lstm',     27,  6, 12,   16, 2, 'fp32', 'RNNT_LSTM_V1'),
    ('lstm_fwd<1,4>',         'lstm_bwd<1,4>',               'lstm',     50,  6, 12,   16, 2, 'fp32', 'RNNT_LSTM_V1'),
    ('lstm_fwd<2,1>',         'lstm_bwd<2,1>',               'lstm',     13,  6, 12,  544, 2, 'fp32', 'RNNT_LSTM_V1'),
    ('lstm_fwd<2,2>',         'lstm_bwd<2,2>',               'lstm',     27,  6, 12,  544, 2, 'fp32', 'RNNT_LSTM_V1'),
    # v2 (lstm.hip, W_hh slice in LDS): H off the multiples of 128.  HS = 16 / 8 / 4 units per workgroup (the largest that divides
    # H), BQ = 1 / 2 / 4 row quads (rows per group <= 4 / 8 / 16), every cell form
    ('lstm_fwd2<16,1,0>',     'lstm_bwd2<16,1,0>',           'lstm',     11,  7, 16,   48, 2, 'fp32', ''),
    ('lstm_fwd2<16,1,1>',     'lstm_bwd2<16,1,1>',           'gru',      11,  7, 16,   48, 2, 'fp32', ''),
    ('lstm_fwd2<16,1,2>',     'lstm_bwd2<16,1,2>',           'rnn_tanh', 11,  7, 16,   48, 2, 'fp32', ''),
    ('lstm_fwd2<16,2,0>',     'lstm_bwd2<16,2,0>',           'lstm',     64,  7, 16,  160, 2, 'fp32', ''),
    ('lstm_fwd2<16,2,1>',     'lstm_bwd2<16,2,1>',           'gru',      64,  7, 16,  160, 2, 'fp32', ''),
    ('lstm_fwd2<16,2,2>',     'lstm_bwd2<16,2,2>',           'rnn_relu', 64,  7, 16,  160, 2, 'fp32', ''),
    ('lstm_fwd2<16,4,0>',     'lstm_bwd2<16,4,0>',           'lstm',     64,  7, 16,  320, 2, 'fp32', ''),
    ('lstm_fwd2<16,4,1>',     'lstm_bwd2<16,4,1>',           'gru',      64,  7, 16,  320, 2, 'fp32', ''),
    ('lstm_fwd2<16,4,2>',     'lstm_bwd2<16,4,2>',           'rnn_tanh', 64,  7, 16,  320, 2, 'fp32', ''),
    ('lstm_fwd2<8,1,0>',      'lstm_bwd2<8,1,0>',            'lstm',      7,  7, 16,   40, 1, 'fp32', ''),
    ('lstm_fwd2<8,1,1>',      'lstm_bwd2<8,1,1>',            'gru',       7,  7, 16,   40, 1, 'fp32', ''),
    ('lstm_fwd2<8,1,2>',      'lstm_bwd2<8,1,2>',            'rnn_relu',  7,  7, 16,   40, 1, 'fp32', ''),
    ('lstm_fwd2<8,2,0>',      'lstm_bwd2<8,2,0>',            'lstm',     29,  7, 16,  200, 2, 'fp32', ''),
    ('lstm_fwd2<8,2,1>',      'lstm_bwd2<8,2,1>',            'gru',      29,  7, 16,  200, 2, 'fp32', ''),
    ('lstm_fwd2<8,2,2>',      'lstm_bwd2<8,2,2>',            'rnn_tanh', 29,  7, 16,  200, 2, 'fp32', ''),
    ('lstm_fwd2<8,4,0>',      'lstm_bwd2<8,4,0>',            'lstm',     61,  7, 16,  200, 2, 'fp32', ''),
    ('lstm_fwd2<8,4,1>',      'lstm_bwd2<8,4,1>',            'gru',      61,  7, 16,  200, 2, 'fp32', ''),
    ('lstm_fwd2<8,4,2>',      'lstm_bwd2<8,4,2>',            'rnn_relu', 61,  7, 16,  200, 2, 'fp32', ''),
    ('lstm_fwd2<4,1,0>',      'lstm_bwd2<4,1,0>',            'lstm',     10,  7, 16,   20, 2, 'fp32', ''),
    ('lstm_fwd2<4,1,1>',      'lstm_bwd2<4,1,1>',            'gru',      10,  7, 16,   20, 2, 'fp32', ''),
    ('lstm_fwd2<4,1,2>',      'lstm_bwd2<4,1,2>',            'rnn_tanh', 10,  7, 16,   20, 2, 'fp32', ''),
    ('lstm_fwd2<4,2,0>',      'lstm_bwd2<4,2,0>',            'lstm',     27,  7, 16,  100, 2, 'fp32', ''),
    ('lstm_fwd2<4,2,1>',      'lstm_bwd2<4,2,1>',            'gru',      27,  7, 16,  100, 2, 'fp32', ''),
    ('lstm_fwd2<4,2,2>',      'lstm_bwd2<4,2,2>',            'rnn_relu', 27,  7, 16,  100, 2, 'fp32', ''),
    ('lstm_fwd2<4,4,0>',      'lstm_bwd2<4,4,0>',            'lstm',     59,  7, 16,  100, 2, 'fp32', ''),
    ('lstm_fwd2<4,4,1>',      'lstm_bwd2<4,4,1>',            'gru',      59,  7, 16,  100, 2, 'fp32', ''),
    ('lstm_fwd2<4,4,2>',      'lstm_bwd2<4,4,2>',            'rnn_tanh', 59,  7, 16,  100, 2, 'fp32', ''),
    # v3 / v4 (lstm.hip, W_hh in registers): ReLU cells and H = 768 / 1024 by default, LSTM / GRU at H <= 640 under RNNT_LSTM_NO_V5.
    # H = 128 / 256 admit only 4- / 8-row groups on 256 CUs (see UNREACHABLE)
    ('lstm_fwd3<1,0,4,4,0>',  'lstm_bwd4<2,1,0,4,4,0>',      'lstm',     13,  7, 24,  128, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<1,1,4,4,0>',  'lstm_bwd4<2,1,1,4,4,0>',      'gru',      13,  7, 24,  128, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<1,2,4,4,0>',  'lstm_bwd4<2,1,2,4,4,0>',      'rnn_relu', 13,  7, 24,  128, 2, 'fp32', ''),
    ('lstm_fwd3<2,0,4,4,0>',  'lstm_bwd4<4,1,0,4,4,0>',      'lstm',      7,  8, 24,  256, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,1,4,4,0>',  'lstm_bwd4<4,1,1,4,4,0>',      'gru',       7,  8, 24,  256, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,2,4,4,0>',  'lstm_bwd4<4,1,2,4,4,0>',      'rnn_relu',  7,  8, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd3<2,0,4,4,0>',  'lstm_bwd4<4,2,0,4,4,0>',      'lstm',     61,  5, 24,  256, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,1,4,4,0>',  'lstm_bwd4<4,2,1,4,4,0>',      'gru',      61,  5, 24,  256, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,2,4,4,0>',  'lstm_bwd4<4,2,2,4,4,0>',      'rnn_relu', 61,  5, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,4,4,0>',  'lstm_bwd4<6,1,0,4,4,0>',      'lstm',     18,  5, 24,  384, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,1,4,4,0>',  'lstm_bwd4<6,1,1,4,4,0>',      'gru',      18,  5, 24,  384, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,2,4,4,0>',  'lstm_bwd4<6,1,2,4,4,0>',      'rnn_relu', 18,  5, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,4,4,0>',  'lstm_bwd4<6,2,0,4,4,0>',      'lstm',     37,  6, 24,  384, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,1,4,4,0>',  'lstm_bwd4<6,2,1,4,4,0>',      'gru',      37,  6, 24,  384, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,2,4,4,0>',  'lstm_bwd4<6,2,2,4,4,0>',      'rnn_relu', 37,  6, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,4,4,0>',  'lstm_bwd4<6,4,0,4,4,0>',      'lstm',     63,  8, 24,  384, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,1,4,4,0>',  'lstm_bwd4<6,4,1,4,4,0>',      'gru',      63,  8, 24,  384, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,2,4,4,0>',  'lstm_bwd4<6,4,2,4,4,0>',      'rnn_relu', 63,  8, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd3<2,0,8,4,0>',  'lstm_bwd4<8,1,0,4,4,0>',      'lstm',     15,  6, 24,  512, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,1,8,4,0>',  'lstm_bwd4<8,1,1,4,4,0>',      'gru',      15,  6, 24,  512, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,2,8,4,0>',  'lstm_bwd4<8,1,2,4,4,0>',      'rnn_relu', 15,  6, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd3<2,0,8,4,0>',  'lstm_bwd4<8,2,0,4,4,0>',      'lstm',     29,  7, 24,  512, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,1,8,4,0>',  'lstm_bwd4<8,2,1,4,4,0>',      'gru',      29,  7, 24,  512, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,2,8,4,0>',  'lstm_bwd4<8,2,2,4,4,0>',      'rnn_relu', 29,  7, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd3<2,0,8,4,0>',  'lstm_bwd4<8,4,0,4,4,0>',      'lstm',     61,  5, 24,  512, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,1,8,4,0>',  'lstm_bwd4<8,4,1,4,4,0>',      'gru',      61,  5, 24,  512, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<2,2,8,4,0>',  'lstm_bwd4<8,4,2,4,4,0>',      'rnn_relu', 61,  5, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,8,5,1>',  'lstm_bwd4<6,1,0,8,5,1>',      'lstm',     15,  7, 24,  640, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,1,8,5,1>',  'lstm_bwd4<6,1,1,8,5,1>',      'gru',      15,  7, 24,  640, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,2,8,5,1>',  'lstm_bwd4<6,1,2,8,5,1>',      'rnn_relu', 15,  7, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,8,5,1>',  'lstm_bwd4<6,2,0,8,5,1>',      'lstm',     29,  8, 24,  640, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,1,8,5,1>',  'lstm_bwd4<6,2,1,8,5,1>',      'gru',      29,  8, 24,  640, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,2,8,5,1>',  'lstm_bwd4<6,2,2,8,5,1>',      'rnn_relu', 29,  8, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,8,5,1>',  'lstm_bwd4<6,4,0,8,5,1>',      'lstm',     61,  6, 24,  640, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,1,8,5,1>',  'lstm_bwd4<6,4,1,8,5,1>',      'gru',      61,  6, 24,  640, 2, 'fp32', 'RNNT_LSTM_NO_V5'),
    ('lstm_fwd3<3,2,8,5,1>',  'lstm_bwd4<6,4,2,8,5,1>',      'rnn_relu', 61,  6, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,8,4,1>',  'lstm_bwd4<6,1,0,8,4,2>',      'lstm',      7,  8, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,1,8,4,1>',  'lstm_bwd4<6,1,1,8,4,2>',      'gru',       7,  8, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,2,8,4,1>',  'lstm_bwd4<6,1,2,8,4,2>',      'rnn_tanh',  7,  8, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,8,4,1>',  'lstm_bwd4<6,2,0,8,4,2>',      'lstm',     15,  5, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,1,8,4,1>',  'lstm_bwd4<6,2,1,8,4,2>',      'gru',      15,  5, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,2,8,4,1>',  'lstm_bwd4<6,2,2,8,4,2>',      'rnn_tanh', 15,  5, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,0,8,4,1>',  'lstm_bwd4<6,4,0,8,4,2>',      'lstm',     31,  7, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,1,8,4,1>',  'lstm_bwd4<6,4,1,8,4,2>',      'gru',      31,  7, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<3,2,8,4,1>',  'lstm_bwd4<6,4,2,8,4,2>',      'rnn_tanh', 31,  7, 24,  768, 2, 'fp32', ''),
    ('lstm_fwd3<4,0,8,4,1>',  'lstm_bwd4<8,1,0,8,4,2>',      'lstm',      7,  6, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,1,8,4,1>',  'lstm_bwd4<8,1,1,8,4,2>',      'gru',       7,  6, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,2,8,4,1>',  'lstm_bwd4<8,1,2,8,4,2>',      'rnn_tanh',  7,  6, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,0,8,4,1>',  'lstm_bwd4<8,2,0,8,4,2>',      'lstm',     15,  7, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,1,8,4,1>',  'lstm_bwd4<8,2,1,8,4,2>',      'gru',      15,  7, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,2,8,4,1>',  'lstm_bwd4<8,2,2,8,4,2>',      'rnn_tanh', 15,  7, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,0,8,4,1>',  'lstm_bwd4<8,4,0,8,4,2>',      'lstm',     31,  5, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,1,8,4,1>',  'lstm_bwd4<8,4,1,8,4,2>',      'gru',      31,  5, 24, 1024, 2, 'fp32', ''),
    ('lstm_fwd3<4,2,8,4,1>',  'lstm_bwd4<8,4,2,8,4,2>',      'rnn_tanh', 31,  5, 24, 1024, 2, 'fp32', ''),
    # v5 (lstm5.hip), fp32 mode; H = 768 / 1024 under RNNT_LSTM_V5_WIDE
    ('lstm_fwd5<1,0,4,4,0>',  'lstm_bwd5f<2,1,0,4,0>',       'lstm',     13,  7, 24,  128, 2, 'fp32', ''),
    ('lstm_fwd5<1,1,4,4,0>',  'lstm_bwd5f<2,1,1,4,0>',       'gru',      13,  7, 24,  128, 2, 'fp32', ''),
    ('lstm_fwd5<1,2,4,4,0>',  'lstm_bwd5f<2,1,2,4,0>',       'rnn_tanh', 13,  7, 24,  128, 2, 'fp32', ''),
    ('lstm_fwd5<2,0,4,4,0>',  'lstm_bwd5f<4,1,0,4,0>',       'lstm',      7,  8, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd5<2,1,4,4,0>',  'lstm_bwd5f<4,1,1,4,0>',       'gru',       7,  8, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd5<2,2,4,4,0>',  'lstm_bwd5f<4,1,2,4,0>',       'rnn_tanh',  7,  8, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd5<2,0,4,4,0>',  'lstm_bwd5f<4,2,0,4,0>',       'lstm',     61,  5, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd5<2,1,4,4,0>',  'lstm_bwd5f<4,2,1,4,0>',       'gru',      61,  5, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd5<2,2,4,4,0>',  'lstm_bwd5f<4,2,2,4,0>',       'rnn_tanh', 61,  5, 24,  256, 2, 'fp32', ''),
    ('lstm_fwd5<3,0,4,4,0>',  'lstm_bwd5f<6,1,0,4,0>',       'lstm',     18,  5, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,1,4,4,0>',  'lstm_bwd5f<6,1,1,4,0>',       'gru',      18,  5, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,2,4,4,0>',  'lstm_bwd5f<6,1,2,4,0>',       'rnn_tanh', 18,  5, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,0,4,4,0>',  'lstm_bwd5f<6,2,0,4,0>',       'lstm',     37,  6, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,1,4,4,0>',  'lstm_bwd5f<6,2,1,4,0>',       'gru',      37,  6, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,2,4,4,0>',  'lstm_bwd5f<6,2,2,4,0>',       'rnn_tanh', 37,  6, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,0,4,4,0>',  'lstm_bwd5f<6,4,0,4,0>',       'lstm',     63,  8, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,1,4,4,0>',  'lstm_bwd5f<6,4,1,4,0>',       'gru',      63,  8, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<3,2,4,4,0>',  'lstm_bwd5f<6,4,2,4,0>',       'rnn_tanh', 63,  8, 24,  384, 2, 'fp32', ''),
    ('lstm_fwd5<2,0,8,4,0>',  'lstm_bwd5f<4,1,0,8,0>',       'lstm',     15,  6, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,1,8,4,0>',  'lstm_bwd5f<4,1,1,8,0>',       'gru',      15,  6, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,2,8,4,0>',  'lstm_bwd5f<4,1,2,8,0>',       'rnn_tanh', 15,  6, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,0,8,4,0>',  'lstm_bwd5f<4,2,0,8,0>',       'lstm',     29,  7, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,1,8,4,0>',  'lstm_bwd5f<4,2,1,8,0>',       'gru',      29,  7, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,2,8,4,0>',  'lstm_bwd5f<4,2,2,8,0>',       'rnn_tanh', 29,  7, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,0,8,4,0>',  'lstm_bwd5f<4,4,0,8,0>',       'lstm',     61,  5, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,1,8,4,0>',  'lstm_bwd5f<4,4,1,8,0>',       'gru',      61,  5, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<2,2,8,4,0>',  'lstm_bwd5f<4,4,2,8,0>',       'rnn_tanh', 61,  5, 24,  512, 2, 'fp32', ''),
    ('lstm_fwd5<3,0,8,5,0>',  'lstm_bwd5<6,1,0,8,5,32,0>',   'lstm',     15,  7, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,1,8,5,0>',  'lstm_bwd5<6,1,1,8,5,32,0>',   'gru',      15,  7, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,2,8,5,0>',  'lstm_bwd5<6,1,2,8,5,32,0>',   'rnn_tanh', 15,  7, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,0,8,5,0>',  'lstm_bwd5<6,2,0,8,5,32,0>',   'lstm',     29,  8, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,1,8,5,0>',  'lstm_bwd5<6,2,1,8,5,32,0>',   'gru',      29,  8, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,2,8,5,0>',  'lstm_bwd5<6,2,2,8,5,32,0>',   'rnn_tanh', 29,  8, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,0,8,5,0>',  'lstm_bwd5<6,4,0,8,5,32,0>',   'lstm',     61,  6, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,1,8,5,0>',  'lstm_bwd5<6,4,1,8,5,32,0>',   'gru',      61,  6, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,2,8,5,0>',  'lstm_bwd5<6,4,2,8,5,32,0>',   'rnn_tanh', 61,  6, 24,  640, 2, 'fp32', ''),
    ('lstm_fwd5<3,0,8,4,0>',  'lstm_bwd5<6,1,0,8,4,64,0>',   'lstm',      7,  8, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,1,8,4,0>',  'lstm_bwd5<6,1,1,8,4,64,0>',   'gru',       7,  8, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,2,8,4,0>',  'lstm_bwd5<6,1,2,8,4,64,0>',   'rnn_tanh',  7,  8, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,0,8,4,0>',  'lstm_bwd5<6,2,0,8,4,64,0>',   'lstm',     15,  5, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,1,8,4,0>',  'lstm_bwd5<6,2,1,8,4,64,0>',   'gru',      15,  5, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,2,8,4,0>',  'lstm_bwd5<6,2,2,8,4,64,0>',   'rnn_tanh', 15,  5, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,0,8,4,0>',  'lstm_bwd5<6,4,0,8,4,64,0>',   'lstm',     31,  7, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,1,8,4,0>',  'lstm_bwd5<6,4,1,8,4,64,0>',   'gru',      31,  7, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,2,8,4,0>',  'lstm_bwd5<6,4,2,8,4,64,0>',   'rnn_tanh', 31,  7, 24,  768, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,0,8,4,0>',  'lstm_bwd5<8,1,0,8,4,64,0>',   'lstm',      7,  6, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,1,8,4,0>',  'lstm_bwd5<8,1,1,8,4,64,0>',   'gru',       7,  6, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,2,8,4,0>',  'lstm_bwd5<8,1,2,8,4,64,0>',   'rnn_tanh',  7,  6, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,0,8,4,0>',  'lstm_bwd5<8,2,0,8,4,64,0>',   'lstm',     15,  7, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,1,8,4,0>',  'lstm_bwd5<8,2,1,8,4,64,0>',   'gru',      15,  7, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,2,8,4,0>',  'lstm_bwd5<8,2,2,8,4,64,0>',   'rnn_tanh', 15,  7, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,0,8,4,0>',  'lstm_bwd5<8,4,0,8,4,64,0>',   'lstm',     31,  5, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,1,8,4,0>',  'lstm_bwd5<8,4,1,8,4,64,0>',   'gru',      31,  5, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,2,8,4,0>',  'lstm_bwd5<8,4,2,8,4,64,0>',   'rnn_tanh', 31,  5, 24, 1024, 2, 'fp32', 'RNNT_LSTM_V5_WIDE'),
    # v5 one-product forms (compute_precision="fp16", half-pair products forced on: T * B >= 1024)
    ('lstm_fwd5<1,0,4,4,1>',  'lstm_bwd5f<2,1,0,4,1>',       'lstm',     13, 79, 40,  128, 2, 'fp16', ''),
    ('lstm_fwd5<1,1,4,4,1>',  'lstm_bwd5f<2,1,1,4,1>',       'gru',      13, 79, 40,  128, 2, 'fp16', ''),
    ('lstm_fwd5<1,2,4,4,1>',  'lstm_bwd5f<2,1,2,4,1>',       'rnn_tanh', 13, 79, 40,  128, 2, 'fp16', ''),
    ('lstm_fwd5<2,0,4,4,1>',  'lstm_bwd5f<4,1,0,4,1>',       'lstm',      7, 147, 40,  256, 2, 'fp16', ''),
    ('lstm_fwd5<2,1,4,4,1>',  'lstm_bwd5f<4,1,1,4,1>',       'gru',       7, 147, 40,  256, 2, 'fp16', ''),
    ('lstm_fwd5<2,2,4,4,1>',  'lstm_bwd5f<4,1,2,4,1>',       'rnn_tanh',  7, 147, 40,  256, 2, 'fp16', ''),
    ('lstm_fwd5<2,0,4,4,1>',  'lstm_bwd5f<4,2,0,4,1>',       'lstm',     61, 17, 40,  256, 2, 'fp16', ''),
    ('lstm_fwd5<2,1,4,4,1>',  'lstm_bwd5f<4,2,1,4,1>',       'gru',      61, 17, 40,  256, 2, 'fp16', ''),
    ('lstm_fwd5<2,2,4,4,1>',  'lstm_bwd5f<4,2,2,4,1>',       'rnn_tanh', 61, 17, 40,  256, 2, 'fp16', ''),
    ('lstm_fwd5<3,0,4,4,1>',  'lstm_bwd5f<6,1,0,4,1>',       'lstm',     39, 27, 40,  384, 1, 'fp16', ''),
    ('lstm_fwd5<3,1,4,4,1>',  'lstm_bwd5f<6,1,1,4,1>',       'gru',      39, 27, 40,  384, 1, 'fp16', ''),
    ('lstm_fwd5<3,2,4,4,1>',  'lstm_bwd5f<6,1,2,4,1>',       'rnn_tanh', 39, 27, 40,  384, 1, 'fp16', ''),
    ('lstm_fwd5<3,0,4,4,1>',  'lstm_bwd5f<6,2,0,4,1>',       'lstm',     62, 17, 40,  384, 1, 'fp16', ''),
    ('lstm_fwd5<3,1,4,4,1>',  'lstm_bwd5f<6,2,1,4,1>',       'gru',      62, 17, 40,  384, 1, 'fp16', ''),
    ('lstm_fwd5<3,2,4,4,1>',  'lstm_bwd5f<6,2,2,4,1>',       'rnn_tanh', 62, 17, 40,  384, 1, 'fp16', ''),
    ('lstm_fwd5<3,0,4,4,1>',  'lstm_bwd5f<6,4,0,4,1>',       'lstm',     63, 17, 40,  384, 2, 'fp16', ''),
    ('lstm_fwd5<3,1,4,4,1>',  'lstm_bwd5f<6,4,1,4,1>',       'gru',      63, 17, 40,  384, 2, 'fp16', ''),
    ('lstm_fwd5<3,2,4,4,1>',  'lstm_bwd5f<6,4,2,4,1>',       'rnn_tanh', 63, 17, 40,  384, 2, 'fp16', ''),
    ('lstm_fwd5<2,0,8,4,1>',  'lstm_bwd5f<4,1,0,8,1>',       'lstm',     31, 34, 40,  512, 1, 'fp16', ''),
    ('lstm_fwd5<2,1,8,4,1>',  'lstm_bwd5f<4,1,1,8,1>',       'gru',      31, 34, 40,  512, 1, 'fp16', ''),
    ('lstm_fwd5<2,2,8,4,1>',  'lstm_bwd5f<4,1,2,8,1>',       'rnn_tanh', 31, 34, 40,  512, 1, 'fp16', ''),
    ('lstm_fwd5<2,0,8,4,1>',  'lstm_bwd5f<4,2,0,8,1>',       'lstm',     61, 17, 40,  512, 1, 'fp16', ''),
    ('lstm_fwd5<2,1,8,4,1>',  'lstm_bwd5f<4,2,1,8,1>',       'gru',      61, 17, 40,  512, 1, 'fp16', ''),
    ('lstm_fwd5<2,2,8,4,1>',  'lstm_bwd5f<4,2,2,8,1>',       'rnn_tanh', 61, 17, 40,  512, 1, 'fp16', ''),
    ('lstm_fwd5<2,0,8,4,1>',  'lstm_bwd5f<4,4,0,8,1>',       'lstm',     61, 17, 40,  512, 2, 'fp16', ''),
    ('lstm_fwd5<2,1,8,4,1>',  'lstm_bwd5f<4,4,1,8,1>',       'gru',      61, 17, 40,  512, 2, 'fp16', ''),
    ('lstm_fwd5<2,2,8,4,1>',  'lstm_bwd5f<4,4,2,8,1>',       'rnn_tanh', 61, 17, 40,  512, 2, 'fp16', ''),
    ('lstm_fwd5<3,0,8,5,1>',  'lstm_bwd5<6,1,0,8,5,32,1>',   'lstm',     31, 34, 40,  640, 1, 'fp16', ''),
    ('lstm_fwd5<3,1,8,5,1>',  'lstm_bwd5<6,1,1,8,5,32,1>',   'gru',      31, 34, 40,  640, 1, 'fp16', ''),
    ('lstm_fwd5<3,2,8,5,1>',  'lstm_bwd5<6,1,2,8,5,32,1>',   'rnn_tanh', 31, 34, 40,  640, 1, 'fp16', ''),
    ('lstm_fwd5<3,0,8,5,1>',  'lstm_bwd5<6,2,0,8,5,32,1>',   'lstm',     61, 17, 40,  640, 1, 'fp16', ''),
    ('lstm_fwd5<3,1,8,5,1>',  'lstm_bwd5<6,2,1,8,5,32,1>',   'gru',      61, 17, 40,  640, 1, 'fp16', ''),
    ('lstm_fwd5<3,2,8,5,1>',  'lstm_bwd5<6,2,2,8,5,32,1>',   'rnn_tanh', 61, 17, 40,  640, 1, 'fp16', ''),
    ('lstm_fwd5<3,0,8,5,1>',  'lstm_bwd5<6,4,0,8,5,32,1>',   'lstm',     61, 17, 40,  640, 2, 'fp16', ''),
    ('lstm_fwd5<3,1,8,5,1>',  'lstm_bwd5<6,4,1,8,5,32,1>',   'gru',      61, 17, 40,  640, 2, 'fp16', ''),
    ('lstm_fwd5<3,2,8,5,1>',  'lstm_bwd5<6,4,2,8,5,32,1>',   'rnn_tanh', 61, 17, 40,  640, 2, 'fp16', ''),
    ('lstm_fwd5<3,0,8,4,1>',  'lstm_bwd5<6,1,0,8,4,64,1>',   'lstm',     19, 54, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,1,8,4,1>',  'lstm_bwd5<6,1,1,8,4,64,1>',   'gru',      19, 54, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,2,8,4,1>',  'lstm_bwd5<6,1,2,8,4,64,1>',   'rnn_tanh', 19, 54, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,0,8,4,1>',  'lstm_bwd5<6,2,0,8,4,64,1>',   'lstm',     39, 27, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,1,8,4,1>',  'lstm_bwd5<6,2,1,8,4,64,1>',   'gru',      39, 27, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,2,8,4,1>',  'lstm_bwd5<6,2,2,8,4,64,1>',   'rnn_tanh', 39, 27, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,0,8,4,1>',  'lstm_bwd5<6,4,0,8,4,64,1>',   'lstm',     63, 17, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,1,8,4,1>',  'lstm_bwd5<6,4,1,8,4,64,1>',   'gru',      63, 17, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<3,2,8,4,1>',  'lstm_bwd5<6,4,2,8,4,64,1>',   'rnn_tanh', 63, 17, 40,  768, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,0,8,4,1>',  'lstm_bwd5<8,1,0,8,4,64,1>',   'lstm',     15, 69, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,1,8,4,1>',  'lstm_bwd5<8,1,1,8,4,64,1>',   'gru',      15, 69, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,2,8,4,1>',  'lstm_bwd5<8,1,2,8,4,64,1>',   'rnn_tanh', 15, 69, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,0,8,4,1>',  'lstm_bwd5<8,2,0,8,4,64,1>',   'lstm',     29, 36, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,1,8,4,1>',  'lstm_bwd5<8,2,1,8,4,64,1>',   'gru',      29, 36, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,2,8,4,1>',  'lstm_bwd5<8,2,2,8,4,64,1>',   'rnn_tanh', 29, 36, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,0,8,4,1>',  'lstm_bwd5<8,4,0,8,4,64,1>',   'lstm',     61, 17, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,1,8,4,1>',  'lstm_bwd5<8,4,1,8,4,64,1>',   'gru',      61, 17, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
    ('lstm_fwd5<4,2,8,4,1>',  'lstm_bwd5<8,4,2,8,4,64,1>',   'rnn_tanh', 61, 17, 40, 1024, 1, 'fp16', 'RNNT_LSTM_V5_WIDE'),
]

# Shapes that once ran a wrong instance, run like the rows (their instances are also declared by a row).
REGRESSION_ROWS = [
    # bi-LSTM H = 520 with 33-64 rows fits neither v2 nor v3 and took v1 with 8-unit slices of 64 rows (MT * NT = 8 tiles for 256
    # threads: half of every slice's units were never computed); it now takes 4-unit slices, two workgroups per CU
    ('lstm_fwd<1,4>',         'lstm_bwd<1,4>',               'lstm',     50,  6, 12,  520, 2, 'fp32', ''),
]

# Past the v5 stash limit: T * B * D * 4H * 4 >= 2^31 goes to the v3 / v4 forms (lstm5_supported), one frame less stays on v5.
STASH_CASES = [
    ("lstm_fwd3<2,0,8,4,0>", "lstm_bwd4<8,4,0,4,4,0>", "lstm", 64, 2048, 80, 512, 2),
    ("lstm_fwd5<2,0,8,4,0>", "lstm_bwd5f<4,4,0,8,0>", "lstm", 64, 2047, 80, 512, 2),
]

# Compiled instances that no shape reaches on a 256-CU device (a launch takes at most 64 rows): pattern, reason.
UNREACHABLE = [
    (r"lstm_(fwd|bwd)<2,4>", "v1: 8-unit slices of 64 rows are 8 tiles for 256 threads; make_plan takes at most 4 (MT * NT <= 4)"),
    (r"lstm_(fwd|bwd)<4,[124]>", "v1 16-unit slices: chosen only where 4- and 8-unit slices need more than 256 / 512 workgroups, and "
                                 "at every such H their LDS exceeds 160 KB"),
    (r"lstm_bwd4<2,[24],[012],4,4,0>", "H = 128: a sync group is 8 workgroups, so up to 16 groups per direction: <= 4 rows per group"),
    (r"lstm_bwd5f<2,[24],[012],4,[01]>", "H = 128: a sync group is 8 workgroups, so up to 16 groups per direction: <= 4 rows per group"),
    (r"lstm_bwd4<4,4,[012],4,4,0>", "H = 256: a sync group is 16 workgroups, so up to 8 groups per direction: <= 8 rows per group"),
    (r"lstm_bwd5f<4,4,[012],4,[01]>", "H = 256: a sync group is 16 workgroups, so up to 8 groups per direction: <= 8 rows per group"),
]


def _row_id(row):
    fwd, bwd, cell, B, T, I, H, D, precision, env = row
    return f"{bwd}-{cell}-B{B}-H{H}-D{D}-{precision}" + (f"-{env}" if env else "")


def declared_instances():
    return {r[0] for r in ROWS + REGRESSION_ROWS} | {r[1] for r in ROWS + REGRESSION_ROWS} | {c[0] for c in STASH_CASES} | \
        {c[1] for c in STASH_CASES}


# ---- the recurrence kernels compiled into librnnt_hip.so (host ELF -> .hip_fatbin -> clang offload bundles -> gfx950 ELF symtab) ----
def _elf_sections(elf):
    assert elf[:4] == b"\x7fELF" and elf[4] == 2 and elf[5] == 1, "64-bit little-endian ELF expected"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    names = secs[shstrndx][4]
    return [(elf[names + s[0]:elf.index(b"\0", names + s[0])].decode(),) + s[1:] for s in secs]


def _bundled_code_objects(fatbin, arch="gfx950"):
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = fatbin.find(magic)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fatbin, pos + len(magic))
        q = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, q)
            triple = fatbin[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if triple.startswith("hip") and triple.endswith(arch):
                yield fatbin[pos + off:pos + off + size]
        pos = fatbin.find(magic, pos + 1)


def compiled_recurrence_instances(lib_path):
    from rnntransducer_amd.ops import recurrence_instance
    blob = open(lib_path, "rb").read()
    fat = [s for s in _elf_sections(blob) if s[0] == ".hip_fatbin"]
    assert fat, f"{lib_path}: no .hip_fatbin section"
    _, _, _, _, off, size, *_ = fat[0]
    found, n_objects = set(), 0
    for co in _bundled_code_objects(blob[off:off + size]):
        n_objects += 1
        for name, typ, _, _, soff, ssize, link, _, _, entsize in _elf_sections(co):
            if typ != 2:   # SHT_SYMTAB
                continue
            strtab = _elf_sections(co)[link][4]
            for i in range(ssize // entsize):
                st_name, st_info = struct.unpack_from("<IB", co, soff + i * entsize)
                sym = co[strtab + st_name:co.index(b"\0", strtab + st_name)].decode()
                if st_info & 15 == 2 and re.search(r"lstm_(fwd|bwd)\w*_kernel", sym):   # STT_FUNC
                    found.add(recurrence_instance(sym))
    assert n_objects > 0, f"{lib_path}: no uncompressed gfx950 code object in .hip_fatbin"
    return found


def test_every_compiled_instance_is_declared_or_unreachable():
    from rnntransducer_amd import _lib
    from rnntransducer_amd.csrc import build
    build.build()
    compiled = compiled_recurrence_instances(_lib.LIB_PATH)
    declared = declared_instances()
    allowed = {n for n in compiled if any(re.fullmatch(p, n) for p, _ in UNREACHABLE)}
    assert not sorted(declared - compiled), f"declared but not compiled (stale rows): {sorted(declared - compiled)}"
    assert not sorted(compiled - declared - allowed), f"compiled but neither tested by a row nor listed as unreachable: " \
                                                     f"{sorted(compiled - declared - allowed)}"
    assert not sorted(declared & allowed), f"listed as unreachable but tested by a row: {sorted(declared & allowed)}"
    for p, reason in UNREACHABLE:
        assert any(re.fullmatch(p, n) for n in compiled), f"UNREACHABLE entry {p!r} matches no compiled instance"
    bwd = [r[1] for r in ROWS]
    assert len(bwd) == len(set(bwd)), "two rows declare the same backward instance"
    print(f"recurrence instances: {len(compiled)} compiled, {len(declared)} tested, {len(allowed)} unreachable")


def test_recurrence_instance_names():
    from rnntransducer_amd.ops import recurrence_instance
    assert recurrence_instance("_ZN4rnnt12_GLOBAL__N_116lstm_fwd5_kernelILi3ELi0ELi8ELi5ELb1EEEvNS_5LstmKE") == "lstm_fwd5<3,0,8,5,1>"
    assert recurrence_instance("_ZN4rnnt12_GLOBAL__N_115lstm_bwd_kernelILi2ELi4EEEvNS_5LstmKE") == "lstm_bwd<2,4>"
    assert recurrence_instance("void rnnt::(anonymous namespace)::lstm_bwd5f_kernel<4, 2, 1, 8, false>(rnnt::LstmK)") == \
        "lstm_bwd5f<4,2,1,8,0>"
    with pytest.raises(ValueError):
        recurrence_instance("_ZN4rnnt12_GLOBAL__N_120zero_padded_rows_kernelEPfPKiiii")


# ---- GPU: every row against torch float64 ----
def _modules(cell, I, H, D, seed):
    from rnntransducer_amd.networks.rnn import HipGRU, HipLSTM, HipRNN
    torch.manual_seed(seed)
    bi = D == 2
    if cell == "lstm":
        ref, hip = nn.LSTM(I, H, 1, batch_first=True, bidirectional=bi), HipLSTM(I, H, 1, bidirectional=bi)
    elif cell == "gru":
        ref, hip = nn.GRU(I, H, 1, batch_first=True, bidirectional=bi), HipGRU(I, H, 1, bidirectional=bi)
    else:
        nl = cell.split("_")[1]
        ref = nn.RNN(I, H, 1, batch_first=True, bidirectional=bi, nonlinearity=nl)
        hip = HipRNN(I, H, 1, bidirectional=bi, nonlinearity=nl)
    ref = ref.double()
    hip.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return ref, hip.cuda()


def _oracle(ref, x, lens, dy):
    from conftest import usable_cores
    torch.set_num_threads(usable_cores())
    T = x.shape[1]
    xr = x.double().requires_grad_(True)
    packed = nn.utils.rnn.pack_padded_sequence(xr, torch.tensor(lens), batch_first=True, enforce_sorted=False)
    out, _ = ref(packed)
    out, _ = nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
    out.backward(dy.double())
    return out.detach(), xr.grad, {k: p.grad for k, p in ref.named_parameters()}


def _hip_run(hip, x_tm, lens, dy_tm):
    """Forward + backward (batch-major results on the CPU) under the launch record."""
    from rnntransducer_amd.ops import lstm_launch_record
    hip.zero_grad()
    _poison_free_memory()
    x_tm = x_tm.cuda().requires_grad_(True)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    with lstm_launch_record() as rec:
        y = hip(x_tm, lens_dev)
        y.backward(dy_tm.cuda())
        torch.cuda.synchronize()
    grads = {k: p.grad.double().cpu() for k, p in hip.named_parameters()}
    return rec.instances, y.detach().transpose(0, 1).double().cpu(), x_tm.grad.transpose(0, 1).double().cpu(), grads


def _assert_padding_zero(y, dx, lens):
    for b, n in enumerate(lens):
        assert torch.all(y[b, n:] == 0), f"output of padded frames, row {b}"
        assert torch.all(dx[b, n:] == 0), f"dx of padded frames, row {b}"


def _assert_fp32_close(y, dx, grads, ref_out, ref_dx, ref_grads):
    e = (y - ref_out).abs().max().item()
    assert e < FWD_ATOL, f"forward err {e}"
    for name, got, want in [("dx", dx, ref_dx)] + [(k, grads[k], ref_grads[k]) for k in ref_grads]:
        scale = max(want.abs().max().item(), 1e-3)
        err = (got - want).abs().max().item()
        assert err < GRAD_RTOL * scale + 1e-6, f"{name}: err {err} scale {scale}"


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS + REGRESSION_ROWS, ids=_row_id)
def test_recurrence_instance_vs_float64(monkeypatch, row):
    fwd, bwd, cell, B, T, I, H, D, precision, env = row
    for name in env.split():
        monkeypatch.setenv(name, "1")
    if precision == "fp16":
        monkeypatch.setenv("RNNT_GEMM_FORCE_HP", "1")   # these shapes are small: put them on the half-pair products (one-product forms)
    ref, hip = _modules(cell, I, H, D, seed=B * 1000 + H)
    hip.compute_precision = precision
    assert hip.effective_precision(T, B) == precision
    g = torch.Generator().manual_seed(H + B)
    lens = [T, 1] + torch.randint(1, T + 1, (B - 2,), generator=g).tolist()
    x = torch.randn(B, T, I, generator=g)
    for b in range(B):
        x[b, lens[b]:] = 0
    dy = torch.randn(B, T, D * H, generator=g)
    ref_out, ref_dx, ref_grads = _oracle(ref, x, lens, dy)
    ran, y, dx, grads = _hip_run(hip, x.transpose(0, 1).contiguous(), lens, dy.transpose(0, 1).contiguous())
    print(f"{_row_id(row)}: {' '.join(ran)}")
    assert ran == [fwd, bwd], f"launched {ran}, the row declares {[fwd, bwd]}"
    _assert_padding_zero(y, dx, lens)
    if precision == "fp32":
        _assert_fp32_close(y, dx, grads, ref_out, ref_dx, ref_grads)
    else:
        e = (y - ref_out).abs().max().item()
        assert e < OUT_ATOL, f"output err {e}"
        for name, got, want in [("dx", dx, ref_dx)] + [(k, grads[k], ref_grads[k]) for k in ref_grads]:
            rn, cos = _grad_stats(got, want)
            assert rn <= GRAD_RNORM and cos >= GRAD_COS, f"{name}: rel norm {rn:.2e}, cosine {cos:.6f}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", STASH_CASES, ids=lambda c: f"T{c[4]}")
def test_stash_limit_selects_the_forms_and_both_sides_match_float64(case):
    """bi-LSTM H = 512, B = 64 at the T where the gate stash reaches 2 GiB (v3 / v4, 64-bit addressing) and one frame below it (v5).
    All 64 rows run; rows 0-1 are checked against float64 with dy = 0 on rows 2.., so the weight gradients come from rows 0-1 only."""
    fwd, bwd, cell, B, T, I, H, D = case
    over = T * B * D * 4 * H * 4 >= 1 << 31
    assert over == fwd.startswith("lstm_fwd3") and (T - 1) * B * D * 4 * H * 4 < 1 << 31 <= (T + 1) * B * D * 4 * H * 4
    ref, hip = _modules(cell, I, H, D, seed=T)
    g = torch.Generator().manual_seed(T)
    lens = [T, T - 613] + torch.randint(1, T + 1, (B - 2,), generator=g).tolist()
    x = torch.randn(B, T, I, generator=g)
    for b in range(B):
        x[b, lens[b]:] = 0
    dy2 = torch.randn(2, T, D * H, generator=g)
    ref_out, ref_dx, ref_grads = _oracle(ref, x[:2], lens[:2], dy2)
    dy_tm = torch.zeros(T, B, D * H)
    dy_tm[:, :2] = dy2.transpose(0, 1)
    ran, y, dx, grads = _hip_run(hip, x.transpose(0, 1).contiguous(), lens, dy_tm)
    print(f"T={T} ({'past' if over else 'below'} the stash limit): {' '.join(ran)}")
    assert ran == [fwd, bwd], f"launched {ran}, expected {[fwd, bwd]}"
    _assert_padding_zero(y, dx, lens)
    assert torch.all(dx[2:] == 0)   # dy = 0 there
    _assert_fp32_close(y[:2], dx[:2], grads, ref_out, ref_dx, ref_grads)
