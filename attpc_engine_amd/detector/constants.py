"""Physical constants baked into the kernels (reference ``detector/constants.py:20-35``;
the reference reads them from scipy's CODATA table -- the exact doubles are repeated in
``csrc/common.hpp`` and checked against scipy in the CPU tests)."""
from scipy.constants import Avogadro, elementary_charge, physical_constants, pi, speed_of_light

NUM_TB: int = 512
MEV_2_JOULE: float = physical_constants["electron volt-joule relationship"][0] * 1.0e6
MEV_2_KG: float = physical_constants["electron volt-kilogram relationship"][0] * 1.0e6
C: float = speed_of_light
E_CHARGE: float = elementary_charge
# track straggling (detector/straggling.py, csrc/straggle_host.hpp): Bohr's K = 4 pi (r_e m_e c^2)^2 in MeV^2 m^2
R_ELECTRON: float = physical_constants["classical electron radius"][0]
M_ELECTRON_MEV: float = physical_constants["electron mass energy equivalent in MeV"][0]
STRAGGLE_K: float = 4.0 * pi * (R_ELECTRON * M_ELECTRON_MEV) * (R_ELECTRON * M_ELECTRON_MEV)
AVOGADRO: float = Avogadro
