"""spmm_arrow CLI — flag-compatible with the reference
(scripts/spmm_arrow_main.py:10-31; console script setup.py:20)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arrow_matrix_amd import arrow_bench
from arrow_matrix_amd.comm import default_comm
from arrow_matrix_amd.common import utils


def main() -> None:
    # Flags and defaults are the reference CLI's (spmm_arrow_main.py:10-31);
    # help text reworded here.
    parser = argparse.ArgumentParser(description='Iterated arrow-SpMM benchmark')
    parser.add_argument('-f', '--path', type=str, default=None,
                        help='decomposed-graph file prefix; omit to run on '
                             'generated synthetic data')
    parser.add_argument('-w', '--width', type=int, default=0,
                        help='arrow width (block height) of the decomposition')
    parser.add_argument('-c', '--features', type=int, default=16,
                        help='feature columns k of the dense operand X')
    parser.add_argument('-b', '--blocked', type=utils.str2bool, nargs="?", default=True,
                        help='block-diagonal decomposition (False: banded '
                             'with +-1 off-diagonal blocks)')
    parser.add_argument('-i', '--device', type=str, default='gpu',
                        help="compute device: 'gpu' (HIP kernels) or 'cpu' "
                             "(scipy, the parity reference)")
    parser.add_argument('-z', '--iterations', type=int, default=1,
                        help='number of X <- A @ X iterations')
    parser.add_argument('-r', '--ranksperside', type=int, default=3,
                        help='synthetic data only: block-rows per matrix')
    parser.add_argument('-m', '--ba_neighbors', type=int, default=3,
                        help='synthetic data only: average neighbors per vertex')
    parser.add_argument('-s', '--slim', type=utils.str2bool, nargs="?", default=True,
                        help='slim layout (one rank per block-row); False '
                             'selects the banded ArrowMPI variant')
    parser.add_argument('-n', '--npy', type=utils.str2bool, nargs="?", default=True,
                        help='load the .npy (indptr/indices/data) format; '
                             'False loads the legacy .npz format')

    # not a reference flag
    parser.add_argument('--damping', type=float, default=None, metavar='D',
                        help='iterate X <- D*A@X + (1-D)*X0 with the initial '
                             'features X0 as residual (default: off, plain '
                             'X <- A@X on fresh features)')

    parser.add_argument('--tol', type=float, default=None, metavar='T',
                        help='with --damping: stop after the first iteration '
                             'whose relative step ||X_new - X_old|| / '
                             '||X_new|| is <= T, and print the steps taken '
                             '(default: off, all -z iterations run)')

    parser.add_argument('--normalize', choices=('row', 'col', 'sym'),
                        default=None,
                        help='normalise the loaded matrix on the device before '
                             'the first step: row (D^-1 A), col (A D^-1, '
                             'PageRank) or sym (D^-1/2 A D^-1/2); default: off')
    parser.add_argument('--normalize-abs', action='store_true',
                        help='with --normalize: use the sums of |a_ij|')

    args = vars(parser.parse_args())
    # off: the printed arguments and the run are what they were without them
    damping = args.pop('damping')
    tol = args.pop('tol')
    normalize = args.pop('normalize')
    normalize_abs = args.pop('normalize_abs')
    if tol is not None and damping is None:
        parser.error('--tol needs --damping')
    if normalize_abs and normalize is None:
        parser.error('--normalize-abs needs --normalize')
    if normalize is not None:
        args['normalize'] = normalize
        if normalize_abs:
            args['normalize_abs'] = True
    if damping is not None:
        args['damping'] = damping
    if tol is not None:
        args['tol'] = tol
    comm = default_comm()
    utils.mpi_print(comm.rank, str(args))

    args['wandb_key'] = os.environ.get('WANDB_API_KEY')
    if args['wandb_key'] is None:
        utils.mpi_print(comm.rank,
                        "Set the WANDB_API_KEY environment variable to start "
                        "logging results to Weights & Biases.")

    arrow_bench.bench_spmm(args['path'],
                           args['width'],
                           args['features'],
                           args['iterations'],
                           args['blocked'],
                           args['device'],
                           args['ranksperside'],
                           args['ba_neighbors'],
                           args['wandb_key'],
                           slim=args['slim'],
                           npy_format=args['npy'],
                           **({} if damping is None
                              else {'damping': damping}),
                           **({} if tol is None else {'tol': tol}),
                           **({} if normalize is None
                              else {'normalize': normalize,
                                    'normalize_abs': normalize_abs}))


if __name__ == '__main__':
    main()
