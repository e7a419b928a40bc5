"""What the host-harness and the GPU tests of the quad body level of the Ant adjoint share.  Test-only."""
import numpy as np

from oracle_lib import golden


def ant_contact_state():
    """(q, qd, act) [1, .]: the state of the contact read-out's recording (ant_con.npz) with the largest contact forces"""
    g = golden("ant_con")
    k = int(np.argmax(np.abs(g["c_force"]).sum(axis=(1, 2))))
    assert np.abs(g["c_force"][k]).sum() > 1.0
    return g["q_in"][k:k + 1].copy(), g["qd_in"][k:k + 1].copy(), g["act_in"][k:k + 1].copy()
