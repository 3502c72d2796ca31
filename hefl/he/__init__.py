from .ckks import CKKSContext, Ciphertext, CtxtTensor, KeyPair, KeyShare
from .linear import LinearTransform
from .pyfhel_compat import Pyfhel, PyCtxt

__all__ = ["CKKSContext", "Ciphertext", "CtxtTensor", "KeyPair", "KeyShare",
           "LinearTransform", "Pyfhel", "PyCtxt"]
