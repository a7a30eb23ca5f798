#!/usr/bin/env python
"""Training entry point — flag surface of the reference's train.py (:19-94) on the MI355X build.

Runs the DCLL half of the reference's loop on the HIP kernels: per training step a batch is encoded to spike planes,
`net.learn(x[t], labels[t])` is called for every timestep (train.py:249-251: forward + local loss + backward + Adam
step per layer per timestep after burn-in, dcll/pytorch_libdcll.py:690-718), learning rates are halved every 1000
steps (:222-229), and every `n_test_interval` steps the test batches are evaluated and `acc_test.npy` /
`parameters_{step}.pth` (reference state-dict keys) are written (:263-303).  Not run: the non-spiking baseline CNN
(ReferenceConvNetwork, networks/__init__.py:21-113 — outside the DCLL path) and tensorboard dumps.
Data: RadioML HDF5 needs h5py (absent here); `--synthetic N` uses the build's seeded constellation generator.
"""
import argparse
import datetime
import os
import pickle
import sys

import numpy as np
import torch

from snn_modulation_classification_amd import parallel
from snn_modulation_classification_amd.data.utils import to_one_hot
from snn_modulation_classification_amd.dcll import pytorch_libdcll
from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
import test_radio_ml as evaluation

_NETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'snn_modulation_classification_amd', 'networks')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='DCLL')
    p.add_argument('--data', type=str, default='RadioML', choices=['MNIST', 'RadioML'], help='which data to use')
    p.add_argument('--radio_ml_data_dir', type=str, default='2018.01', help='folder with the RadioML HDF5 file(s)')
    p.add_argument('--mnist_data_dir', type=str, default='./data', help='folder with the MNIST IDX files (--data MNIST)')
    p.add_argument('--min_snr', type=int, default=6, metavar='N', help='minimum SNR (inclusive)')
    p.add_argument('--max_snr', type=int, default=30, metavar='N', help='maximum SNR (inclusive)')
    p.add_argument('--per_h5_frac', type=float, default=0.5, metavar='N', help='fraction of each HDF5 file to use')
    p.add_argument('--train_frac', type=float, default=0.9, metavar='N', help='train split')
    p.add_argument('--network_spec', type=str, default=os.path.join(_NETS, 'radio_ml_conv.yaml'), metavar='S')
    p.add_argument('--ref_network_spec', type=str, default=os.path.join(_NETS, 'radio_ml_conv_ref.yaml'), metavar='S')
    p.add_argument('--just_ref', action='store_true', help='train only the non-spiking reference network')
    p.add_argument('--I_resolution', type=int, default=128, metavar='N')
    p.add_argument('--Q_resolution', type=int, default=128, metavar='N')
    p.add_argument('--I_bounds', type=float, default=(-1, 1), nargs=2)
    p.add_argument('--Q_bounds', type=float, default=(-1, 1), nargs=2)
    p.add_argument('--restore_path', type=str, metavar='S', help='.pth state-dict to restore')
    p.add_argument('--burnin', type=int, default=50, metavar='N')
    p.add_argument('--batch_size', type=int, default=64, metavar='N')
    p.add_argument('--batch_size_test', type=int, default=64, metavar='N')
    p.add_argument('--n_steps', type=int, default=10000, metavar='N', help='number of steps to train')
    p.add_argument('--no_save', type=evaluation.str2bool_like_reference, default=False, metavar='N')
    p.add_argument('--seed', type=int, default=1, metavar='S')
    p.add_argument('--n_test_interval', type=int, default=20, metavar='N')
    p.add_argument('--n_test_samples', type=int, default=128, metavar='N')
    p.add_argument('--n_iters', type=int, default=1024, metavar='N')
    p.add_argument('--n_iters_test', type=int, default=1024, metavar='N')
    p.add_argument('--optim_type', type=str, default='Adam', metavar='S')
    p.add_argument('--loss_type', type=str, default='SmoothL1Loss', metavar='S')
    p.add_argument('--learning_rates', type=float, default=[1e-6], nargs='+', metavar='N')
    p.add_argument('--ref_lr', type=float, default=1e-3, metavar='N')
    p.add_argument('--alpha', type=float, default=.92, metavar='N')
    p.add_argument('--alphas', type=float, default=.85, metavar='N')
    p.add_argument('--alpharp', type=float, default=.65, metavar='N')
    p.add_argument('--arp', type=float, default=0, metavar='N')
    p.add_argument('--random_tau', type=evaluation.str2bool_like_reference, default=True)
    p.add_argument('--beta', type=float, default=.95, metavar='N')
    p.add_argument('--lc_ampl', type=float, default=0.5, metavar='N')
    p.add_argument('--netscale', type=float, default=1., metavar='N')
    p.add_argument('--comment', type=str, default='')
    p.add_argument('--output', type=str, default='results')
    # additions of this build
    p.add_argument('--synthetic', type=int, default=0, metavar='N', help='use N synthetic test windows')
    p.add_argument('--eval_only', action='store_true', help='run the periodic evaluation once and save parameters')
    p.add_argument('--host_encoding', action='store_true',
                   help='encode the training batches with the host iq2spiketrain loop (the reference\'s way) instead of on '
                        'the device')
    p.add_argument('--any_sequence_path', action='store_true',
                   help='opt in: the test phase of a network without a geometry-specialised sequence kernel '
                        '(sequence_supported() False, e.g. --data MNIST with mnist_conv.yaml, or RadioML on a 24x24 plane) runs '
                        'ConvNetwork.test_sequence_any (k_lif_seq_any) where it serves every layer, instead of net.test per timestep')
    p.add_argument('--wide_sequence_path', action='store_true',
                   help='opt in: --any_sequence_path through dcll_conv_lif_sequence_wide — the test phase of a network without a '
                        'geometry-specialised sequence kernel runs ConvNetwork.test_sequence_any(wide=True): k_lif_seq_wide for '
                        'layers of 33-64 output channels (--netscale up to 2), k_lif_seq_any up to 32; one process only; ignored '
                        'with a notice where the network is not served.  Measured on an MI355X against the per-step loop, five '
                        'alternating fresh processes, min-max ms per sequence: radio_ml_conv.yaml at netscale 2 on 16x16, T = 128: '
                        '343.10-343.87 -> 167.33-167.67 at B = 512 (2.05x), but NOT faster at B = 64: 62.59-62.97 -> 82.96-83.44 '
                        '(one workgroup per sample leaves CUs idle below 256 samples); mnist_conv.yaml at netscale 2, T = 50: '
                        '15.78-15.98 -> 13.62-13.76 at B = 32 (1.15x), 79.00-79.60 -> 29.03-29.09 at B = 512 (2.72x) (DESIGN 4.1e; '
                        'experiments/seq_wide_timing.py)')
    p.add_argument('--band_sequence_path', type=int, nargs='?', const=0, default=None, metavar='N',
                   help='opt in: the test phase of a network without a geometry-specialised sequence kernel runs '
                        'ConvNetwork.test_sequence_any(bands=N) — dcll_conv_lif_sequence_bands, N workgroups per sample, each on a '
                        'band of output rows for all T (k_lif_seq_band; N omitted or 0: the library\'s rule per layer; 1: '
                        'dcll_conv_lif_sequence_wide itself).  Serves layers of up to 64 output channels, and planes whose '
                        'per-sample state is beyond one workgroup\'s LDS (radio_ml_conv.yaml on 48x48).  One process only; ignored '
                        'with a notice where the network is not served.  Wins over --any_sequence_path and --wide_sequence_path '
                        'where more than one is given (DESIGN 4.1f; experiments/seq_band_timing.py)')
    p.add_argument('--tile_sequence_path', type=int, nargs='*', default=None, metavar='N',
                   help='opt in, TY TX: the test phase of a network without a geometry-specialised sequence kernel runs '
                        'ConvNetwork.test_sequence_any(tiles=(TY, TX)) — dcll_conv_lif_sequence_tiles, TY x TX workgroups per '
                        'sample, each on a tile of the output plane for all T (k_lif_seq_tile; both omitted or 0 0: the library\'s '
                        'rule per layer, derived from the LDS formula alone; TX = 1: dcll_conv_lif_sequence_bands itself with TY '
                        'bands).  Serves the layers no band count serves: radio_ml_conv.yaml at netscale 2 on planes wider than '
                        '16 pixels, at netscale 1 on planes that are no multiple of 8x32.  One process only; ignored with a notice '
                        'where the network is not served.  Wins over --any_sequence_path, --wide_sequence_path and '
                        '--band_sequence_path.  Measured on an MI355X, T = 128, per-step loop -> the rule, ms per sequence: netscale 2 '
                        'on 24x40, B = 64: 251.56-254.38 -> 184.56-185.38 (faster, 1.36x), B = 512: 1878.74-1884.58 -> '
                        '1435.98-1438.96 (faster, 1.31x); netscale 1 on 100x100, B = 64: 923.29-936.81 -> 460.72-462.17 (faster, '
                        '2.00x); NOT faster at netscale 2 on 128x128, B = 64: 2608.86-2617.72 -> 3135.56-3149.17, and at netscale 1 '
                        'on 48x48, B = 64: 68.86-69.88 -> 114.26-115.33 (the band rule; every tile plan is slower still) '
                        '(DESIGN 4.1g; experiments/seq_tile_timing.py)')
    p.add_argument('--slab_sequence_path', type=int, nargs='*', default=None, metavar='N',
                   help='opt in, TY TX: the test phase of a network without a geometry-specialised sequence kernel runs '
                        'ConvNetwork.test_sequence_any(slabs=(TY, TX)) — dcll_conv_lif_sequence_slabs: layers of MORE than 64 output '
                        'channels (--netscale above 2) in slabs of 64, TY x TX tiles per (sample, slab), each workgroup on a tile of '
                        'the output plane and a slab of channels for all T (k_lif_seq_slab; both omitted or 0 0: the library\'s rule '
                        'per layer, derived from the LDS formula alone); layers of at most 64 channels go through '
                        'dcll_conv_lif_sequence_tiles itself.  One process only; ignored with a notice where the network is not '
                        'served.  Wins over --any_sequence_path, --wide_sequence_path, --band_sequence_path and --tile_sequence_path.  '
                        'Measured on an MI355X, T = 128, per-step loop -> the rule, ms per sequence, radio_ml_conv.yaml on 16x16: NOT faster at netscale 3 (B = 64: 111.59-112.27 -> 139.58-139.99; B = 512: 728.19-729.73 -> 1042.14-1043.32) and NOT faster at netscale 4 (B = 64: 179.94-180.63 -> 259.04-259.78; B = 512: 1258.31-1261.64 -> 1997.00-2004.39): the path is served, not quicker (DESIGN 4.1h; experiments/slab_timing.py)')
    p.add_argument('--any_learning_path', action='store_true',
                   help='opt in: every layer\'s weight gradient of the learning step runs on k_bwd_wgrad_any (fp32 MFMA; any '
                        'plain conv layer with c_out <= 32 and a kernel up to 16x16, which lifts the default path\'s 64-tap '
                        'limit) where ConvNetwork.backward_any_supported() holds; ignored with a notice elsewhere.  Whether it '
                        'is faster than the default dispatch is not measured yet (DESIGN 4.2a; experiments/bwd_any_timing.py)')
    p.add_argument('--wide_learning_path', action='store_true',
                   help='opt in: every layer\'s weight gradient of the learning step runs through dcll_conv_lif_backward_wide — '
                        'k_bwd_wgrad_wide (fp32 MFMA, two 32-row M tiles per wave) for layers of 33-64 output channels (--netscale up '
                        'to 2), k_bwd_wgrad_any up to 32 — where ConvNetwork.backward_wide_supported() holds; ignored with a notice '
                        'elsewhere and together with --any_learning_path / --w3_step_path.  Measured on an MI355X against the same tree '
                        'without the flag, five alternating fresh processes, min-max ms per net.learn timestep: radio_ml_conv.yaml at '
                        'netscale 2 on 16x16, T = 128: 7.035-7.072 -> 0.752-0.757 at B = 64 (9.3-9.4x), 19.03-19.16 -> 4.049-4.071 at '
                        'B = 512 (4.7x); mnist_conv.yaml at netscale 2, T = 50: 2.178-2.193 -> 0.441-0.444 at B = 32 (4.9-5.0x), '
                        '10.51-10.55 -> 2.411-2.423 at B = 512 (4.3-4.4x); every layer\'s open backward call is faster, none slower; '
                        'the per-step forward of such layers stays on the default kernels (DESIGN 4.2d; '
                        'profiles/r20_bwd_wide_timing.txt; experiments/bwd_wide_timing.py)')
    p.add_argument('--slab_learning_path', action='store_true',
                   help='opt in: every layer\'s weight gradient of the learning step runs through dcll_conv_lif_backward_slab — '
                        'k_bwd_wgrad_slab (fp32 MFMA, one slab of 64 output channels per workgroup) for layers of more than 64 output '
                        'channels (--netscale above 2), k_bwd_wgrad_wide for 33-64, k_bwd_wgrad_any up to 32 — where '
                        'ConvNetwork.backward_slab_supported() holds; ignored with a notice elsewhere and together with '
                        '--any_learning_path / --wide_learning_path / --w3_step_path.  Measured on an MI355X against the same tree without the flag, five alternating fresh processes, min-max ms per net.learn timestep, radio_ml_conv.yaml on 16x16, T = 128: netscale 3: 15.55-15.57 -> 1.552-1.563 at B = 64 (9.9-10.0x), 42.04-42.09 -> 9.245-9.313 at B = 512 (4.5x); netscale 4: 27.45-27.49 -> 2.332-2.356 at B = 64 (11.7-11.8x), 74.35-74.56 -> 14.78-14.90 at B = 512 (5.0x); every layer\'s open backward call is faster, none slower; the votes of the free-running arms are NOT equal (another summation order under Adam); the forward of such layers stays on the default kernels (DESIGN 4.2f; '
                        'experiments/slab_timing.py)')
    p.add_argument('--band_learning_path', nargs='?', type=int, const=0, default=None, metavar='N',
                   help='opt in: every layer\'s weight gradient of the learning step runs through dcll_conv_lif_backward_bands — '
                        'k_bwd_wgrad_band (fp32 MFMA, a sample cut into bands of conv-output rows, so LDS does not grow with the '
                        'plane height) for the layers whose sample --slab_learning_path cannot stage (netscale 2 on 24x40, 48x48 and '
                        'larger planes, kernels above 64 taps there), that path\'s kernels for the layers it serves — where '
                        'ConvNetwork.backward_bands_supported() holds.  N: exactly N bands per sample (default: the library\'s rule).  '
                        'Ignored with a notice elsewhere and together with --any_learning_path / --wide_learning_path / '
                        '--slab_learning_path / --w3_step_path; combines with the per-step forward paths.  Measured on an MI355X against '
                        'the same tree without the flag, five alternating fresh processes, min-max ms per net.learn timestep, '
                        'radio_ml_conv.yaml: netscale 2 on 24x40 (--slab_step_path in both arms) 9.788-9.810 -> 1.745-1.756 at B = 64 '
                        '(5.6x), 52.08-52.24 -> 11.11-11.22 at B = 512 (4.6-4.7x); netscale 2 on 128x128 41.69-41.81 -> 9.60-9.75 at '
                        'B = 16 (4.3-4.4x); NOT faster at netscale 1 on 48x48, B = 64: 1.215-1.237 -> 1.369-1.398 (the default dispatch '
                        'there is the tiled MFMA kernel of the headline network) (DESIGN 4.2h; profiles/r27_bwd_band_timing.txt; '
                        'experiments/bwd_band_timing.py)')
    p.add_argument('--any_step_path', action='store_true',
                   help='opt in: every per-step layer call (net.test per timestep, every learning timestep) runs k_lif_step_any '
                        '(one fp32-MFMA launch with the traces and the pooling fused in; any plain conv layer with c_out <= 32 and '
                        'a kernel up to 16x16) where ConvNetwork.step_any_supported() holds; ignored with a notice elsewhere.  '
                        'The sequence paths are not affected.  Not yet measured against the default path (DESIGN 4.2b; '
                        'experiments/step_any_timing.py)')
    p.add_argument('--wide_step_path', action='store_true',
                   help='opt in: every per-step layer call (net.test per timestep, every learning timestep) runs through '
                        'dcll_conv_lif_step_wide — k_lif_step_wide (k_lif_step_any\'s form with two 32-row M tiles) for layers of 33-64 '
                        'output channels (--netscale up to 2), k_lif_step_any up to 32 — where ConvNetwork.step_wide_supported() '
                        'holds; ignored with a notice elsewhere and together with --any_step_path / --w3_step_path; combines with '
                        '--wide_learning_path.  The sequence paths are not affected.  Measured on an MI355X against the same tree '
                        'without the flag, --wide_learning_path in both arms, five alternating fresh processes, min-max ms per '
                        'timestep: radio_ml_conv.yaml at netscale 2 on 16x16: net.test 0.491-0.497 -> 0.426-0.459 at B = 64 '
                        '(1.07-1.17x), 2.672-2.683 -> 1.374-1.378 at B = 512 (1.94-1.95x); net.learn 0.756-0.759 -> 0.693-0.695 at '
                        'B = 64 (1.09-1.10x), 4.350-4.528 -> 2.961-2.987 at B = 512 (1.46-1.53x); mnist_conv.yaml at netscale 2: '
                        'net.learn 2.395-2.413 -> 1.263-1.288 at B = 512 (1.86-1.91x), but NOT faster at B = 32: 0.440-0.441 -> '
                        '0.445-0.447 (one workgroup per sample leaves CUs idle in the layers that are not split) (DESIGN 4.2e; '
                        'profiles/r21_step_wide_timing.txt; experiments/step_wide_timing.py)')
    p.add_argument('--slab_step_path', action='store_true',
                   help='opt in: every per-step layer call (net.test per timestep, every learning timestep) runs through '
                        'dcll_conv_lif_step_slab — k_lif_step_slab (k_lif_step_wide\'s chains over bands of rows x slabs of 64 output '
                        'channels) for layers of more than 64 output channels (--netscale above 2) and for planes whose padded '
                        'eps1 image exceeds a workgroup\'s LDS, dcll_conv_lif_step_wide\'s kernels for the layers that call serves '
                        '— where ConvNetwork.step_slab_supported() holds; ignored with a notice elsewhere and together with '
                        '--any_step_path / --wide_step_path / --w3_step_path; combines with --slab_learning_path.  The sequence '
                        'paths are not affected (DESIGN 4.2g; experiments/step_slab_timing.py)')
    p.add_argument('--w3_step_path', action='store_true',
                   help='opt in (radio_ml_conv_ref.yaml: the 64-channel layers with kernel (1,3), padding (0,1), pooling (1,2)): '
                        'every per-step layer call runs k_lif_step_w3 (traces, fp32-MFMA chains and pooling in one launch) and '
                        'every learning step takes the weight gradient of the 64 -> 64 layers from k_bwd_wgrad_w3, where '
                        'ConvNetwork.w3_step_supported() holds; ignored with a notice elsewhere.  The sequence paths are not '
                        'affected.  Measured on an MI355X, (16,128) plane, five alternating fresh processes, min-max: net.test '
                        '0.850-0.861 -> 0.490-0.504 ms per timestep at B = 64 (1.7x), 2.839-2.847 -> 1.005-1.013 ms at B = 512 '
                        '(2.8x); net.learn 19.41-19.51 -> 0.933-0.945 ms at B = 64 (20.5-20.9x), 44.21-44.29 -> 4.151-4.164 ms at '
                        'B = 512 (10.6-10.7x); the step call of every layer and the backward call of every 64 -> 64 layer are '
                        'faster, none slower; the first layer\'s open backward call is 1.30 ms of the 4.15 at B = 512, of which the '
                        'generic k_bwd_wgrad is 0.48 ms: see --w3_first_wgrad.  Table: profiles/r13_w3_learn_timing.txt')
    p.add_argument('--w3_first_wgrad', action='store_true',
                   help='opt in, effective only together with --w3_step_path on a network it serves: the first layer (c_in 1 -> '
                        '64) takes its weight gradient from k_bwd_wgrad_w3f (a register-only streaming reduction of the dv plane) '
                        'instead of the generic k_bwd_wgrad; ignored with a notice elsewhere.  Measured on an MI355X, (16,128) plane, '
                        'five alternating fresh processes, min-max: that kernel 479.6 -> 52.2 us at B = 512 (0.83 of the copy rate), '
                        'layer 0\'s open backward call 1294.6-1298.8 -> 865.1-867.9 us, net.learn 4.083-4.110 -> 3.665-3.688 ms '
                        '(1.11-1.12x); at B = 64 the call 176.6-179.9 -> 102.9-104.9 us, net.learn 1.116-1.185 -> 1.034-1.442 ms: '
                        'ranges overlap, not claimed faster.  Table: profiles/r14_w3f_wgrad_timing.txt')
    p.add_argument('--w3_dv_path', action='store_true',
                   help='opt in, effective only together with --w3_step_path on a network it serves: every layer\'s backward takes '
                        'its dv plane from k_bwd_dv_w3 (a streaming form of k_bwd_dv for the (1,2) pooling: two pooled positions per '
                        'thread, readout weights in registers) instead of the generic k_bwd_dv; the plane, and with it every '
                        'gradient, is bit-identical; ignored with a notice elsewhere.  Measured on an MI355X, (16,128) plane, with --w3_step_path '
                        '--w3_first_wgrad in both arms, five alternating fresh processes, min-max: net.learn 3.689-3.709 -> 2.263-2.271 ms '
                        'per timestep at B = 512 (1.62-1.64x), 1.050-1.088 -> 0.883-0.913 ms at B = 64 (1.15-1.23x); layer 0\'s dv kernel '
                        '829.5 -> 100.1 us at B = 512 (0.85 of the copy rate); the open backward call of every one of the seven layers is '
                        'faster at both batch sizes, none slower.  Table: profiles/r15_w3_dv_timing.txt')
    p.add_argument('--pool_dv_path', action='store_true',
                   help='opt in: every learning step\'s backward call goes through dcll_conv_lif_backward_ex with DCLL_BWD_POOL_DV, '
                        'so a layer that pools (pool sizes 1-3) takes its dv plane from k_bwd_dv_pool (a streaming form of k_bwd_dv: a '
                        'thread owns a pooled window, readout weights in registers) instead of the generic k_bwd_dv; the plane, and with '
                        'it every gradient, is bit-identical.  Combines with every learning and step path except --w3_step_path '
                        '(which has --w3_dv_path); ignored with a notice there and where no layer of the network pools.  '
                        'Table: profiles/r28_pool_dv_timing.txt')
    p.add_argument('--native_optim_path', action='store_true',
                   help='opt in: with --optim_type Adamax or AdamW (through the layer API also SGD and amsgrad) the learning timestep '
                        'stays on the native path — the update is applied by k_grad_reduce_optim in the launch that finishes the weight '
                        'gradients, on the state tensors of the torch optimizer — instead of running under autograd with one '
                        'optimizer.step() per slice.  Combines with every learning, step and dv path; ignored with a notice under '
                        '--optim_type Adam (already native) and for optimizers that are not served (NAdam, RAdam, RMSprop).  '
                        'Measured on an MI355X, radio_ml_conv.yaml on 16x16, five alternating fresh processes per arm, min-max '
                        'net.learn ms per timestep, flag off -> on: Adamax 1.483-1.945 -> 0.208-0.211 at B = 64 (7.0-9.4x), 1.281-3.130 -> '
                        '0.636-0.683 at B = 512 (1.9-4.9x); AdamW 1.399-1.781 -> 0.208-0.241 at B = 64 (5.8-8.6x), 1.537-1.791 -> '
                        '0.635-0.640 at B = 512 (2.4-2.8x): faster at all four points.  Table: profiles/r29_optim_timing.txt')
    p.add_argument('--gpus', type=int, default=1, metavar='N',
                   help='ranks (one process per GPU): every batch is sharded over them, the local-learning gradients are '
                        'averaged over the ranks every timestep (one bucketed all-reduce)')
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.gpus > 1 and not parallel.under_launcher():
        # plain start: become the launcher of one fresh process per rank (never touches the GPU itself)
        return sys.exit(parallel.spawn_local_ranks(args.gpus, argv=[os.path.abspath(__file__)] +
                                                   (sys.argv[1:] if argv is None else list(argv))))
    rank, local_rank, world = parallel.init_process_group()
    if world > 1 and torch.cuda.is_available():
        pytorch_libdcll.device = 'cuda:%d' % parallel.local_device(local_rank)
        torch.cuda.set_device(parallel.local_device(local_rank))
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if args.data == 'MNIST':
        return main_mnist(args)
    if args.just_ref:
        sys.exit('ReferenceConvNetwork (plain CNN baseline) is outside the DCLL hot path and not part of this build.')
    stamp = datetime.datetime.now().strftime('%b%d_%H-%M-%S')
    out_dir = os.path.join(args.output, args.data, stamp)
    if world > 1:                                  # one results directory for the job: rank 0 names it
        names = [out_dir]
        torch.distributed.broadcast_object_list(names, src=0)
        out_dir = names[0]
    os.makedirs(out_dir, exist_ok=world > 1)
    if rank == 0:
        print('out dir: {}'.format(out_dir))
    if rank != 0:
        args.no_save = True                        # every rank trains its shard; rank 0 alone writes files

    im_dims = (1, args.Q_resolution, args.I_resolution)
    target_size = evaluation.TARGET_SIZE
    opt = getattr(torch.optim, args.optim_type)
    opt_param = {'betas': [0.0, args.beta], 'weight_decay': 10.0}
    loss = getattr(torch.nn, args.loss_type)
    convs = load_network_spec(args.network_spec)
    # sized for this rank's shard of a batch (identical initial weights / time constants on every rank: their RNG draws
    # do not depend on the batch size)
    lo, hi = parallel.shard_range(args.batch_size_test if args.eval_only else args.batch_size, rank, world)
    net = ConvNetwork(args, im_dims, max(hi - lo, 1), convs, target_size,
                      act=torch.nn.Sigmoid(), loss=loss, opt=opt, opt_param=opt_param,
                      learning_rates=args.learning_rates, burnin=args.burnin)
    if args.restore_path:
        print('-' * 80)
        if not os.path.isfile(args.restore_path):
            print('ERROR: Cannot load `%s`.' % args.restore_path)
            print('File does not exist! Aborting load...')
        else:
            net.load_state_dict(torch.load(args.restore_path))
            print('Loaded the SNN model from `%s`.' % args.restore_path)
        print('-' * 80)
    net = net.to(pytorch_libdcll.device)
    net.reset(True)
    _opt_in_paths(net, args)
    parallel.freeze_startup_heap()          # (a full GC pass over the start-up heap costs ~100 ms inside the T-loop)

    if not args.no_save:
        with open(os.path.join(out_dir, 'args.txt'), 'w') as f:
            f.write(str(args))
        with open(os.path.join(out_dir, 'args.pkl'), 'wb') as f:
            pickle.dump(vars(args), f)

    from snn_modulation_classification_amd.data.utils import IQEncoder, iq2spiketrain
    n_test = int(np.ceil(float(args.n_test_samples) / args.batch_size_test))
    gen_train = train_data = None
    if args.synthetic:
        test_batches = evaluation.synthetic_modulation_batches(args.synthetic, args.batch_size_test, args.max_snr,
                                                               max(args.n_iters_test, 128), args.seed)[:n_test]
    else:
        # the reference's data path (train.py:134-141, :196-207): per-(class, SNR) RadioML blocks, interleaved;
        # n_test fixed test batches drawn once, training batches from a shuffling loader that restarts when exhausted
        from snn_modulation_classification_amd.data.load_radio_ml import get_radio_ml_loader
        kw = dict(data_dir=args.radio_ml_data_dir, min_snr=args.min_snr, max_snr=args.max_snr,
                  per_h5_frac=args.per_h5_frac, train_frac=args.train_frac)
        train_data = get_radio_ml_loader(args.batch_size, train=True, **kw)
        gen_train = iter(train_data)
        gen_test = iter(get_radio_ml_loader(args.batch_size_test, train=False, **kw))
        test_batches = [next(gen_test) for _ in range(n_test)]
        n_test = len(test_batches)
    use_sequence = net.sequence_supported()
    device_encoding = not args.host_encoding
    encoder = IQEncoder(args.I_resolution, args.Q_resolution, args.I_bounds, args.Q_bounds,
                        device=pytorch_libdcll.device) if (use_sequence or device_encoding) else None
    import time
    t_train, n_train = 0.0, 0

    # --any_sequence_path / --wide_sequence_path / --band_sequence_path [N] / --tile_sequence_path [TY TX] / --slab_sequence_path [TY TX]: a
    # network without a specialised sequence kernel is tested on ConvNetwork.test_sequence_any (one process only; several ranks keep
    # evaluate_batch's sharded per-step evaluation)
    seq_any = _opt_in_sequence(net, args, use_sequence, world)

    def evaluate_batch_any(samples, labels1h):
        """The per-step branch of evaluate_batch (host-encoded planes, reference test_radio_ml.py:142-146) with its T-loop replaced
        by ConvNetwork.test_sequence_any on the same planes -> per-layer accuracies."""
        T = args.n_iters_test
        spikes, targets = iq2spiketrain(samples, labels1h, out_w=args.I_resolution, out_h=args.Q_resolution,
                                        min_I=args.I_bounds[0], max_I=args.I_bounds[1], min_Q=args.Q_bounds[0],
                                        max_Q=args.Q_bounds[1], max_duration=T)
        net.reset()
        net.eval()
        net.test_sequence_any(torch.Tensor(spikes).to(pytorch_libdcll.device)[:T], **seq_any)
        return net.accuracy(torch.as_tensor(np.asarray(targets), dtype=torch.float32))

    def run_tests(step):
        net.batch_size = max(1, np.diff(parallel.shard_range(args.batch_size_test, rank, world))[0])
        acc = np.empty([len(test_batches), len(net.dcll_slices)])
        for i, (samples, labels) in enumerate(test_batches):
            if seq_any is not None:
                acc[i, :] = evaluate_batch_any(samples, to_one_hot(labels, target_size))
                continue
            acc[i, :], _ = evaluation.evaluate_batch(net, args, samples, to_one_hot(labels, target_size), encoder,
                                                     use_sequence)
        net.batch_size = max(1, np.diff(parallel.shard_range(args.batch_size, rank, world))[0])
        if rank == 0:
            print('[TEST]  Step {} \t Accuracy {} \t Ref {}'.format(str(step).zfill(5), np.mean(acc, axis=0), 'N/A'))
        return acc

    if args.eval_only:
        acc_test = run_tests(0)[None]
    else:
        n_tests_total = int(np.ceil(float(args.n_steps) / args.n_test_interval))
        acc_test = np.empty([n_tests_total, n_test, len(net.dcll_slices)])
        st_kw = dict(out_w=args.I_resolution, out_h=args.Q_resolution, min_I=args.I_bounds[0], max_I=args.I_bounds[1],
                     min_Q=args.Q_bounds[0], max_Q=args.Q_bounds[1], max_duration=args.n_iters, gs_stdev=0)
        for step in range(args.n_steps):
            if ((step + 1) % 1000) == 0:                      # reference :222-229
                for sl in net.dcll_slices:
                    sl.optimizer.param_groups[-1]['lr'] /= 2
                net.dcll_slices[-1].optimizer2.param_groups[-1]['lr'] /= 2
                print('Adjusting learning rates')
            if gen_train is None:
                snr = int(np.random.randint(args.min_snr // 2, args.max_snr // 2 + 1) * 2)
                samples, labels = evaluation.synthetic_modulation_batches(
                    args.batch_size, args.batch_size, snr, max(args.n_iters, 128), args.seed + 7919 * (step + 1))[0]
            else:
                try:
                    samples, labels = next(gen_train)
                except StopIteration:                         # reference :231-235
                    gen_train = iter(train_data)
                    samples, labels = next(gen_train)
                if samples.shape[0] != args.batch_size:       # ragged last batch: the state is sized for batch_size
                    gen_train = iter(train_data)
                    samples, labels = next(gen_train)
            net.global_batch = samples.shape[0]               # (the gradient all-reduce weighs the shards by it)
            enc_pos = dict(start=0, total=samples.shape[0])   # my samples' positions in the whole batch (exact quantisation)
            if world > 1:                                     # my contiguous shard of the batch
                a, b = parallel.shard_range(samples.shape[0], rank, world)
                samples, labels = samples[a:b], labels[a:b]
                enc_pos['start'] = a
            t_step = time.perf_counter()
            labels1h = to_one_hot(labels, target_size)
            net.reset()
            net.train()
            if device_encoding:
                # raw IQ to the GPU, iq2spiketrain's quantisation as a kernel (same random crop draw), burn-in steps on
                # the fused sequence kernels, learning steps on device-built planes
                dev = pytorch_libdcll.device
                cells = encoder(samples.to(dev), args.n_iters, **enc_pos)
                y = torch.as_tensor(np.asarray(labels1h), dtype=torch.float32).to(dev)
                net.learn_sequence(cells, y)
                labels_spikes = y.unsqueeze(0).expand(args.n_iters, -1, -1)
            else:
                spikes, targets = iq2spiketrain(samples, labels1h, **st_kw)
                input_spikes = torch.Tensor(spikes).to(pytorch_libdcll.device)
                labels_spikes = torch.as_tensor(np.asarray(targets), dtype=torch.float32).to(pytorch_libdcll.device)
                for t in range(args.n_iters):
                    net.learn(x=input_spikes[t], labels=labels_spikes[t])
            acc_train = net.accuracy(labels_spikes)           # (reads the per-step argmax back: ends the step's GPU work)
            t_train += time.perf_counter() - t_step
            n_train += samples.shape[0] * world
            if rank == 0:
                print('[TRAIN] Step {} \t Accuracy {} \t {:.0f} windows/s incl. encoding'.format(
                    str(step).zfill(5), acc_train, n_train / t_train))
            if (step % args.n_test_interval) == 0:
                acc_test[step // args.n_test_interval] = run_tests(step)
                if not args.no_save:
                    np.save(os.path.join(out_dir, 'acc_test.npy'), acc_test)
                    save_path = os.path.join(out_dir, 'parameters_{}.pth'.format(step))
                    torch.save(net.cpu().state_dict(), save_path)
                    net.to(pytorch_libdcll.device)
                    print('-' * 80)
                    print('Saved network parameters to `%s`.' % save_path)
                    print('-' * 80)
        if world > 1:
            parallel.barrier()
            torch.distributed.destroy_process_group()
        return out_dir

    # --eval_only: the periodic evaluation block of the reference (train.py:263-303) once, then save
    if not args.no_save:
        np.save(os.path.join(out_dir, 'acc_test.npy'), acc_test)
        save_path = os.path.join(out_dir, 'parameters_{}.pth'.format(0))
        torch.save(net.cpu().state_dict(), save_path)
        net.to(pytorch_libdcll.device)
        print('-' * 80)
        print('Saved network parameters to `%s`.' % save_path)
        print('-' * 80)
    return out_dir


def _tile_sequence_arg(args, flag='tile_sequence_path'):
    """--tile_sequence_path / --slab_sequence_path [TY TX] -> (ty, tx), None where the flag is absent (both omitted: (0, 0))"""
    t = getattr(args, flag, None)
    if t is None:
        return None
    if len(t) not in (0, 2):
        raise SystemExit('--%s takes no value or two (TY TX)' % flag)
    return (int(t[0]), int(t[1])) if t else (0, 0)


def _opt_in_sequence(net, args, use_sequence, world=1):
    """The keyword arguments of ConvNetwork.test_sequence_any for the test phase, None where it does not run there.  It runs where a
    sequence flag is given, the caller's test phase does not run the specialised sequence kernels (use_sequence False), there is one
    process, and the flag's call serves every layer.  --slab_sequence_path [TY TX] (dcll_conv_lif_sequence_slabs) wins over
    --tile_sequence_path [TY TX] (..._tiles) over --band_sequence_path [N] (..._bands) over --wide_sequence_path (..._wide) over
    --any_sequence_path; every flag that was given and is not the one served prints a notice, --any_sequence_path keeps silent."""
    plan = lambda t: '%d x %d tiles' % t if t != (0, 0) else 'any tile plan'
    bands = getattr(args, 'band_sequence_path', None)
    # flag, test_sequence_any's keyword, its value (None: not given), whether the value is valid, how a notice words the value
    flags = [('slab', 'slabs', _tile_sequence_arg(args, 'slab_sequence_path'), lambda t: min(t) >= 0, plan),
             ('tile', 'tiles', _tile_sequence_arg(args), lambda t: min(t) >= 0, plan),
             ('band', 'bands', bands, lambda n: n >= 0, lambda n: '%d bands' % n if n else 'any band count'),
             ('wide', 'wide', True if args.wide_sequence_path else None, lambda v: True, None)]
    chosen = None
    for flag, kw, value, valid, words in flags:
        if value is None:
            continue
        if use_sequence:
            why = 'the network runs its geometry-specialised sequence kernels'
        elif world > 1:
            why = 'several ranks keep the sharded per-step evaluation'
        elif not valid(value) or not net.sequence_any_supported(**{kw: value}):
            why = 'dcll_conv_lif_sequence_%s does not serve every layer of this network' % kw + (' with ' + words(value) if words else '')
        else:
            chosen = chosen or {kw: value}
            continue
        print('--%s_sequence_path ignored: %s' % (flag, why))
    if chosen is None and args.any_sequence_path and not use_sequence and world == 1 and net.sequence_any_supported():
        chosen = {}
    return chosen


def _opt_in_paths(net, args):
    """The flags of the opt-in per-step and learning paths, in the order of paths.PATHS: `net.<switch> = <the flag's value>` where the
    network accepts it, else a notice and the path as it was (paths.refusal: what it rides on, another path in effect, a layer that
    is not served)."""
    from snn_modulation_classification_amd import paths
    for p in paths.PATHS:
        v = getattr(args, p.name, None)
        if v is None or v is False:
            continue
        v = True if p.key != 'band' or v == 0 else v          # (--band_learning_path [N]; 0 bands: the library's rule)
        if p.name == 'pool_dv_path' and not any(tuple(s.dclllayer.pooling) != (1, 1) for s in net.dcll_slices) and not net.w3_step_path:
            print('--pool_dv_path ignored: no layer of this network pools')
        elif p.name == 'native_optim_path' and all(s._plain_adam() for s in net.dcll_slices):
            print('--native_optim_path ignored: every optimizer of this network is plain Adam, which the native step serves already')
        else:
            why = paths.refusal(net, p, v)
            if why:
                print('--%s ignored: %s' % (p.name, paths.notice_text(p, why, v, given=bool(getattr(args, p.rides_on or '', False)))))
                continue
            setattr(net, p.name, v)
            if p.name == 'native_optim_path' and not all(s._native_learning() is not None for s in net.dcll_slices):
                net.native_optim_path = False
                print('--native_optim_path ignored: the learning step of this network is not native whatever its optimizer (loss type, '
                      'layer options or DCLL_NATIVE_LEARNING=0 keep it under autograd)')


def main_mnist(args):
    """--data MNIST (reference train.py:118-131): 28x28 images as frozen Poisson spike trains (image2spiketrain,
    gain 100), 10 classes, any conv spec that fits 28x28 (networks/mnist_conv.yaml), per-step protocol for learning
    and for the periodic test.  Images from the IDX files under --mnist_data_dir, or `--synthetic N` random images."""
    from snn_modulation_classification_amd.data.utils import image2spiketrain
    if args.just_ref:
        sys.exit('ReferenceConvNetwork (plain CNN baseline) is outside the DCLL hot path and not part of this build.')
    stamp = datetime.datetime.now().strftime('%b%d_%H-%M-%S')
    out_dir = os.path.join(args.output, args.data, stamp)
    os.makedirs(out_dir)
    print('out dir: {}'.format(out_dir))
    im_dims, target_size = (1, 28, 28), 10
    opt = getattr(torch.optim, args.optim_type)
    opt_param = {'betas': [0.0, args.beta], 'weight_decay': 10.0}
    loss = getattr(torch.nn, args.loss_type)
    convs = load_network_spec(args.network_spec)
    net = ConvNetwork(args, im_dims, args.batch_size, convs, target_size, act=torch.nn.Sigmoid(), loss=loss, opt=opt,
                      opt_param=opt_param, learning_rates=args.learning_rates, burnin=args.burnin)
    if args.restore_path and os.path.isfile(args.restore_path):
        net.load_state_dict(torch.load(args.restore_path))
        print('Loaded the SNN model from `%s`.' % args.restore_path)
    net = net.to(pytorch_libdcll.device)
    net.reset(True)
    _opt_in_paths(net, args)
    seq_any = _opt_in_sequence(net, args, net.sequence_supported())
    parallel.freeze_startup_heap()          # (a full GC pass over the start-up heap costs ~100 ms inside the T-loop)
    n_test = int(np.ceil(float(args.n_test_samples) / args.batch_size_test))
    if args.synthetic:
        g = torch.Generator().manual_seed(args.seed)
        def batches(n, bs):
            return [(torch.rand(bs, 28, 28, generator=g), torch.randint(0, 10, (bs,), generator=g)) for _ in range(n)]
        test_batches = batches(n_test, args.batch_size_test)
        train_data = batches(max(1, args.synthetic // args.batch_size), args.batch_size)
    else:
        from snn_modulation_classification_amd.data.load_mnist import get_mnist_loader
        train_data = get_mnist_loader(args.batch_size, train=True, data_dir=args.mnist_data_dir)
        gen_test = iter(get_mnist_loader(args.batch_size_test, train=False, data_dir=args.mnist_data_dir))
        test_batches = [next(gen_test) for _ in range(n_test)]
    gen_train = iter(train_data)
    st_train = dict(input_shape=im_dims, gain=100, min_duration=args.n_iters - 1, max_duration=args.n_iters)
    st_test = dict(input_shape=im_dims, gain=100, min_duration=args.n_iters_test - 1, max_duration=args.n_iters_test)
    dev = pytorch_libdcll.device

    def spikes_of(samples, labels, kw):
        sp, tg = image2spiketrain(samples.numpy(), to_one_hot(labels, target_size), **kw)
        return (torch.Tensor(sp).to(dev), torch.as_tensor(np.asarray(tg), dtype=torch.float32).to(dev))

    n_tests_total = int(np.ceil(float(args.n_steps) / args.n_test_interval))
    acc_test = np.empty([n_tests_total, n_test, len(net.dcll_slices)])
    for step in range(args.n_steps):
        if ((step + 1) % 1000) == 0:
            for sl in net.dcll_slices:
                sl.optimizer.param_groups[-1]['lr'] /= 2
            net.dcll_slices[-1].optimizer2.param_groups[-1]['lr'] /= 2
            print('Adjusting learning rates')
        try:
            samples, labels = next(gen_train)
        except StopIteration:
            gen_train = iter(train_data)
            samples, labels = next(gen_train)
        if samples.shape[0] != args.batch_size:
            gen_train = iter(train_data)
            samples, labels = next(gen_train)
        x, y = spikes_of(samples, labels, st_train)
        net.batch_size = args.batch_size
        net.reset()
        net.train()
        for t in range(args.n_iters):
            net.learn(x=x[t], labels=y[t])
        print('[TRAIN] Step {} \t Accuracy {}'.format(str(step).zfill(5), net.accuracy(y)))
        if (step % args.n_test_interval) == 0:
            net.batch_size = args.batch_size_test
            for i, (ts, tl) in enumerate(test_batches):
                tx, ty = spikes_of(ts, tl, st_test)
                net.reset()
                net.eval()
                if seq_any is not None:
                    net.test_sequence_any(tx[:args.n_iters_test], **seq_any)
                else:
                    for t in range(args.n_iters_test):
                        net.test(x=tx[t])
                acc_test[step // args.n_test_interval, i, :] = net.accuracy(ty)
            print('[TEST]  Step {} \t Accuracy {} \t Ref N/A'.format(
                str(step).zfill(5), np.mean(acc_test[step // args.n_test_interval], axis=0)))
            if not args.no_save:
                np.save(os.path.join(out_dir, 'acc_test.npy'), acc_test)
                save_path = os.path.join(out_dir, 'parameters_{}.pth'.format(step))
                torch.save(net.cpu().state_dict(), save_path)
                net.to(dev)
                print('Saved network parameters to `%s`.' % save_path)
    return out_dir


if __name__ == '__main__':
    main()
