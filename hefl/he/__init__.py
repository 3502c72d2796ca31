from .ckks import CKKSContext, Ciphertext, CtxtTensor, KeyPair, KeyShare
from .pyfhel_compat import Pyfhel, PyCtxt

__all__ = ["CKKSContext", "Ciphertext", "CtxtTensor", "KeyPair", "KeyShare",
           "Pyfhel", "PyCtxt"]
