"""argparse validators used by the distance CLI (reference: tracs/utils.py:86-99)."""
import argparse


def check_positive_int(value):
    ivalue = int(value)
    if ivalue <= 0:
        raise argparse.ArgumentTypeError("%s is an invalid positive int value" % value)
    return ivalue


def check_positive_float(value):
    fvalue = float(value)
    if fvalue <= 0:
        raise argparse.ArgumentTypeError("%s is an invalid positive float value" % value)
    return fvalue


def check_nearest_k(value):
    """--nearest K: 1 <= K <= 1024 (tracs_nearest's bound)."""
    ivalue = int(value)
    if ivalue < 1 or ivalue > 1024:
        raise argparse.ArgumentTypeError("%s is an invalid --nearest value: K must be in [1, 1024]" % value)
    return ivalue
