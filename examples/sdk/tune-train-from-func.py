"""The experiment of the reference notebook ``examples/v1beta1/sdk/tune-train-from-func.ipynb`` as a
script: CMA-ES tunes ``lr`` (0.1-0.2) and ``num_epoch`` (10-15) of the Keras MNIST CNN, trained with
plain SGD at batch 64 for 70 steps per epoch, over 12 trials, 2 in parallel, through
``KatibClient.tune()``. The objective is ``katib_amd.workloads.mnist_tfcnn.train_mnist_model``: it
runs on the fused HIP step when the trial has a GPU and on the torch module otherwise, and prints
``accuracy=... - loss=...`` per epoch for the StdOut collector. BASELINE.md B8 / B9 are the
notebook's own figures for this experiment.

    python3 examples/sdk/tune-train-from-func.py [--gpus 1]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from katib_amd import sdk as katib  # noqa: E402
from katib_amd.workloads.mnist_tfcnn import train_mnist_model  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="tune-mnist")
    ap.add_argument("--gpus", type=int, default=1, help="GPUs per trial (0: the torch module on the CPU)")
    ap.add_argument("--max-trial-count", type=int, default=12)
    ap.add_argument("--parallel-trial-count", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=3600)
    args = ap.parse_args(argv)

    parameters = {
        "lr": katib.search.double(min=0.1, max=0.2),
        "num_epoch": katib.search.int(min=10, max=15),
    }
    client = katib.KatibClient()
    client.tune(
        name=args.name,
        objective=train_mnist_model,
        parameters=parameters,
        algorithm_name="cmaes",
        objective_metric_name="accuracy",
        additional_metric_names=["loss"],
        max_trial_count=args.max_trial_count,
        parallel_trial_count=args.parallel_trial_count,
        resources_per_trial={"gpu": args.gpus},
    )
    try:
        client.wait_for_experiment_condition(args.name, timeout=args.timeout)
        print(f"Katib Experiment is Succeeded: {client.is_experiment_succeeded(args.name)}\n")
        best = client.get_optimal_hyperparameters(args.name)
        print("Current Optimal Trial\n")
        print(best)
    finally:
        client.manager.shutdown()  # the in-process scheduler and its trial runtime
    return best


if __name__ == "__main__":
    main()
