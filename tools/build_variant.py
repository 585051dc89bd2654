"""Build a tuning variant of the library next to the product one:  python tools/build_variant.py NAME -DFLAG ...
-> build_variants/NAME.so (git-ignored), built with the product FLAGS plus the given ones."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tropical_cyclone_risk_amd import build as b
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.makedirs(os.path.join(root, 'build_variants'), exist_ok=True)
print(b.build(force=True, verbose=True, flags=sys.argv[2:], out=os.path.join(root, 'build_variants', sys.argv[1] + '.so')))
