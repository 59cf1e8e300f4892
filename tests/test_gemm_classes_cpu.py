"""The launch classes of the split-f16 GEMM (tests/gemm_class_helpers.py), checked without a GPU: the enumeration against
the committed list below - a change of the form rule shows up as a diff of that list -, one representative per class,
the exactness of the operands tests/test_gemm_classes_gpu.py launches them with, and the sensitivity of its value check
to the product count."""
import exact_helpers as X
import gemm_class_helpers as G

# Every class key the grid reaches, sorted.  Re-generate after a change of the rule:
#   python -c "import sys; sys.path.insert(0, 'tests'); import gemm_class_helpers as G; [print(f'    \"{k}\",') for k in G.enumerate_classes()[0]]"
CLASS_KEYS = (
    "refused hi=0 wide=0 plain=1 K=chainable Kp%64=0",
    "refused hi=0 wide=0 plain=1 K=chainable Kp%64=32",
    "refused hi=0 wide=0 plain=1 K=one-launch Kp%64=0",
    "refused hi=0 wide=0 plain=1 K=one-launch Kp%64=32",
    "refused hi=0 wide=0 plain=1 K=short Kp%64=0",
    "refused hi=0 wide=0 plain=1 K=short Kp%64=32",
    "refused hi=0 wide=1 plain=0 K=chainable Kp%64=0",
    "refused hi=0 wide=1 plain=0 K=chainable Kp%64=32",
    "refused hi=0 wide=1 plain=0 K=one-launch Kp%64=0",
    "refused hi=0 wide=1 plain=0 K=one-launch Kp%64=32",
    "refused hi=0 wide=1 plain=0 K=short Kp%64=0",
    "refused hi=0 wide=1 plain=0 K=short Kp%64=32",
    "refused hi=0 wide=1 plain=1 K=chainable Kp%64=0",
    "refused hi=0 wide=1 plain=1 K=chainable Kp%64=32",
    "refused hi=0 wide=1 plain=1 K=one-launch Kp%64=0",
    "refused hi=0 wide=1 plain=1 K=one-launch Kp%64=32",
    "refused hi=0 wide=1 plain=1 K=short Kp%64=0",
    "refused hi=0 wide=1 plain=1 K=short Kp%64=32",
    "refused hi=1 wide=0 plain=0 K=one-launch Kp%64=0",
    "refused hi=1 wide=0 plain=0 K=one-launch Kp%64=32",
    "refused hi=1 wide=0 plain=1 K=chainable Kp%64=0",
    "refused hi=1 wide=0 plain=1 K=chainable Kp%64=32",
    "refused hi=1 wide=0 plain=1 K=one-launch Kp%64=0",
    "refused hi=1 wide=0 plain=1 K=one-launch Kp%64=32",
    "refused hi=1 wide=0 plain=1 K=short Kp%64=0",
    "refused hi=1 wide=0 plain=1 K=short Kp%64=32",
    "refused hi=1 wide=1 plain=0 K=chainable Kp%64=0",
    "refused hi=1 wide=1 plain=0 K=chainable Kp%64=32",
    "refused hi=1 wide=1 plain=0 K=one-launch Kp%64=0",
    "refused hi=1 wide=1 plain=0 K=one-launch Kp%64=32",
    "refused hi=1 wide=1 plain=0 K=short Kp%64=32",
    "refused hi=1 wide=1 plain=1 K=chainable Kp%64=0",
    "refused hi=1 wide=1 plain=1 K=chainable Kp%64=32",
    "refused hi=1 wide=1 plain=1 K=one-launch Kp%64=0",
    "refused hi=1 wide=1 plain=1 K=one-launch Kp%64=32",
    "refused hi=1 wide=1 plain=1 K=short Kp%64=32",
    "tile=128 prod=3 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=128 prod=3 K=longk plain=- wide=0 out=both gelu=0",
    "tile=128 prod=3 K=longk plain=- wide=0 out=both gelu=1",
    "tile=128 prod=3 K=longk plain=- wide=0 out=f32 gelu=1",
    "tile=128 prod=3 K=longk plain=- wide=0 out=split gelu=0",
    "tile=128 prod=3 K=longk plain=- wide=0 out=split gelu=1",
    "tile=128 prod=3 K=short plain=- wide=0 out=both gelu=0",
    "tile=128 prod=3 K=short plain=- wide=0 out=both gelu=1",
    "tile=128 prod=3 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=128 prod=3 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=128 prod=3 K=short plain=- wide=0 out=split gelu=0",
    "tile=128 prod=3 K=short plain=- wide=0 out=split gelu=1",
    "tile=192 prod=1 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=192 prod=1 K=short plain=- wide=0 out=both gelu=0",
    "tile=192 prod=1 K=short plain=- wide=0 out=both gelu=1",
    "tile=192 prod=1 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=192 prod=1 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=192 prod=1 K=short plain=- wide=0 out=split gelu=0",
    "tile=192 prod=1 K=short plain=- wide=0 out=split gelu=1",
    "tile=192 prod=2 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=chained plain=A wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=chained plain=AO wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=chained plain=AW wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=chained plain=AWO wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=chained plain=O wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=chained plain=W wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=chained plain=WO wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=- wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=- wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=- wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=- wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=- wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=- wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=- wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=- wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=- wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=- wide=1 out=split gelu=1",
    "tile=192 prod=2 K=short plain=A wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=A wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=A wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=A wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=A wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=A wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=A wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=A wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=A wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=A wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=A wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=A wide=1 out=split gelu=1",
    "tile=192 prod=2 K=short plain=AO wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=AO wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=AO wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=AO wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=AO wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=AO wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=AO wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=AO wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=AO wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=AO wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=AO wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=AO wide=1 out=split gelu=1",
    "tile=192 prod=2 K=short plain=AW wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=AW wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=AW wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=AW wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=AW wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=AW wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=AW wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=AW wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=AW wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=AW wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=AW wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=AW wide=1 out=split gelu=1",
    "tile=192 prod=2 K=short plain=AWO wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=AWO wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=AWO wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=AWO wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=AWO wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=AWO wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=AWO wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=AWO wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=AWO wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=AWO wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=AWO wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=AWO wide=1 out=split gelu=1",
    "tile=192 prod=2 K=short plain=O wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=O wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=O wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=O wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=O wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=O wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=O wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=O wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=O wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=O wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=O wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=O wide=1 out=split gelu=1",
    "tile=192 prod=2 K=short plain=W wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=W wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=W wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=W wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=W wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=W wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=W wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=W wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=W wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=W wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=W wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=W wide=1 out=split gelu=1",
    "tile=192 prod=2 K=short plain=WO wide=0 out=both gelu=0",
    "tile=192 prod=2 K=short plain=WO wide=0 out=both gelu=1",
    "tile=192 prod=2 K=short plain=WO wide=0 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=WO wide=0 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=WO wide=0 out=split gelu=0",
    "tile=192 prod=2 K=short plain=WO wide=0 out=split gelu=1",
    "tile=192 prod=2 K=short plain=WO wide=1 out=both gelu=0",
    "tile=192 prod=2 K=short plain=WO wide=1 out=both gelu=1",
    "tile=192 prod=2 K=short plain=WO wide=1 out=f32 gelu=0",
    "tile=192 prod=2 K=short plain=WO wide=1 out=f32 gelu=1",
    "tile=192 prod=2 K=short plain=WO wide=1 out=split gelu=0",
    "tile=192 prod=2 K=short plain=WO wide=1 out=split gelu=1",
    "tile=192 prod=3 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=192 prod=3 K=short plain=- wide=0 out=both gelu=0",
    "tile=192 prod=3 K=short plain=- wide=0 out=both gelu=1",
    "tile=192 prod=3 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=192 prod=3 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=192 prod=3 K=short plain=- wide=0 out=split gelu=0",
    "tile=192 prod=3 K=short plain=- wide=0 out=split gelu=1",
    "tile=256 prod=1 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=256 prod=1 K=short plain=- wide=0 out=both gelu=0",
    "tile=256 prod=1 K=short plain=- wide=0 out=both gelu=1",
    "tile=256 prod=1 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=256 prod=1 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=256 prod=1 K=short plain=- wide=0 out=split gelu=0",
    "tile=256 prod=1 K=short plain=- wide=0 out=split gelu=1",
    "tile=256 prod=2 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=chained plain=A wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=chained plain=AO wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=chained plain=AW wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=chained plain=AWO wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=chained plain=O wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=chained plain=W wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=chained plain=WO wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=- wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=- wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=- wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=- wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=- wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=- wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=- wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=- wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=- wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=- wide=1 out=split gelu=1",
    "tile=256 prod=2 K=short plain=A wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=A wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=A wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=A wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=A wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=A wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=A wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=A wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=A wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=A wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=A wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=A wide=1 out=split gelu=1",
    "tile=256 prod=2 K=short plain=AO wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=AO wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=AO wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=AO wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=AO wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=AO wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=AO wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=AO wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=AO wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=AO wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=AO wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=AO wide=1 out=split gelu=1",
    "tile=256 prod=2 K=short plain=AW wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=AW wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=AW wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=AW wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=AW wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=AW wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=AW wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=AW wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=AW wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=AW wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=AW wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=AW wide=1 out=split gelu=1",
    "tile=256 prod=2 K=short plain=AWO wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=AWO wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=AWO wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=AWO wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=AWO wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=AWO wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=AWO wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=AWO wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=AWO wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=AWO wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=AWO wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=AWO wide=1 out=split gelu=1",
    "tile=256 prod=2 K=short plain=O wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=O wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=O wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=O wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=O wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=O wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=O wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=O wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=O wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=O wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=O wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=O wide=1 out=split gelu=1",
    "tile=256 prod=2 K=short plain=W wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=W wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=W wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=W wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=W wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=W wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=W wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=W wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=W wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=W wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=W wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=W wide=1 out=split gelu=1",
    "tile=256 prod=2 K=short plain=WO wide=0 out=both gelu=0",
    "tile=256 prod=2 K=short plain=WO wide=0 out=both gelu=1",
    "tile=256 prod=2 K=short plain=WO wide=0 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=WO wide=0 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=WO wide=0 out=split gelu=0",
    "tile=256 prod=2 K=short plain=WO wide=0 out=split gelu=1",
    "tile=256 prod=2 K=short plain=WO wide=1 out=both gelu=0",
    "tile=256 prod=2 K=short plain=WO wide=1 out=both gelu=1",
    "tile=256 prod=2 K=short plain=WO wide=1 out=f32 gelu=0",
    "tile=256 prod=2 K=short plain=WO wide=1 out=f32 gelu=1",
    "tile=256 prod=2 K=short plain=WO wide=1 out=split gelu=0",
    "tile=256 prod=2 K=short plain=WO wide=1 out=split gelu=1",
    "tile=256 prod=3 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=256 prod=3 K=short plain=- wide=0 out=both gelu=0",
    "tile=256 prod=3 K=short plain=- wide=0 out=both gelu=1",
    "tile=256 prod=3 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=256 prod=3 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=256 prod=3 K=short plain=- wide=0 out=split gelu=0",
    "tile=256 prod=3 K=short plain=- wide=0 out=split gelu=1",
    "tile=64 prod=1 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=64 prod=1 K=short plain=- wide=0 out=both gelu=0",
    "tile=64 prod=1 K=short plain=- wide=0 out=both gelu=1",
    "tile=64 prod=1 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=64 prod=1 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=64 prod=1 K=short plain=- wide=0 out=split gelu=0",
    "tile=64 prod=1 K=short plain=- wide=0 out=split gelu=1",
    "tile=64 prod=3 K=chained plain=- wide=0 out=f32 gelu=0",
    "tile=64 prod=3 K=short plain=- wide=0 out=both gelu=0",
    "tile=64 prod=3 K=short plain=- wide=0 out=both gelu=1",
    "tile=64 prod=3 K=short plain=- wide=0 out=f32 gelu=0",
    "tile=64 prod=3 K=short plain=- wide=0 out=f32 gelu=1",
    "tile=64 prod=3 K=short plain=- wide=0 out=split gelu=0",
    "tile=64 prod=3 K=short plain=- wide=0 out=split gelu=1",
)

SMALL_MN = 1 << 17           # representatives up to this M * N are evaluated in full on the CPU, the others bounded


def test_enumeration_is_the_committed_list():
    reps, count = G.enumerate_classes()
    keys = tuple(reps)
    missing, new = sorted(set(CLASS_KEYS) - set(keys)), sorted(set(keys) - set(CLASS_KEYS))
    assert not missing and not new, f"classes gone: {missing}; classes not in the committed list: {new}"
    assert keys == CLASS_KEYS
    acc, ref = G.accepted(), G.refused()
    # what the grid found: every tile the rule knows in the fp32-accurate mode; the reduced-precision mode has no 128-row
    # tile (its only one was the one-launch long-K kernel, which the rule refuses in that mode)
    tiles = {hi: sorted({int(k.split()[0][5:]) for k, c in acc if G.is_hi(c) == hi}) for hi in (False, True)}
    print(f"{len(acc)} accepted and {len(ref)} refused classes over {sum(count.values())} calls; tiles: fp32-accurate "
          f"{tiles[False]}, reduced precision {tiles[True]}")
    assert tiles[False] == [64, 128, 192, 256] and tiles[True] == [64, 192, 256]
    # both sides of the 256-tile threshold in each mode, every product count, chained and one-launch long K
    for hi in (False, True):
        mine = [k for k, c in acc if G.is_hi(c) == hi]
        assert any("K=chained" in k for k in mine) and any("K=short" in k for k in mine)
    assert {k.split()[1] for k, _ in acc} == {"prod=1", "prod=2", "prod=3"}
    assert any("K=longk" in k for k, c in acc if not G.is_hi(c))
    assert not any("K=longk" in k for k, c in acc if G.is_hi(c)), "reduced precision has no one-launch long-K kernel"
    # the two k-step widths of the reduced-precision big tiles, and of its chained form
    for tile in (192, 256):
        for prod in (1, 2):
            assert any(k.startswith(f"tile={tile} prod={prod} K=short") for k, _ in acc)
    assert any(k.startswith("tile=192 prod=1 K=chained") or k.startswith("tile=256 prod=1 K=chained") for k, _ in acc)
    assert any(" prod=2 K=chained" in k for k, _ in acc)


def test_every_class_has_one_representative_of_its_own():
    reps, count = G.enumerate_classes()
    assert set(reps) == set(count) and all(n > 0 for n in count.values())
    for k, c in reps.items():
        assert G.class_key(c) == k
        assert (G.call_form(c) < 0) == k.startswith("refused")
    calls = list(reps.values())
    assert len(set(calls)) == len(calls)                      # pairwise distinct calls, hence (class_key is a function) classes
    # the representative is the smallest member: no grid call of the class has a smaller M * N * Kp
    best = {}
    for c in G.grid():
        k = G.class_key(c)
        best[k] = min(best.get(k, 1 << 62), c.M * c.N * c.Kp)
    assert all(best[k] == c.M * c.N * c.Kp for k, c in reps.items())
    shapes = sorted({(c.M, c.N, c.Kp) for _, c in G.accepted()})
    print(f"{len(shapes)} representative shapes: {shapes}")


def test_representative_operands_stay_exact():
    """per representative shape and mode: planes that reconstruct the input, no f16 subnormal, non-zero lo planes, and
    max sum |term| < 2^24 granules - evaluated where M * N is small, bounded from the planes where it is not.  A shape
    that cannot be made exact is reported by name."""
    failures, lines = [], []
    todo = sorted({(c.M, c.N, c.Kp, G.is_hi(c), c.gelu) for _, c in G.accepted()})
    planes = {}
    for M, N, Kp, hi, gelu in todo:
        if (M, N, Kp) not in planes:
            a, w, b, r = G.operands(M, N, Kp)
            pa, pw = X.split_model(a), X.split_model(w, G.W_SCALE)
            X.check_planes(a, pa[0], pa[1], 1.0, "A")
            X.check_planes(w, pw[0], pw[1], 1.0 / G.W_SCALE, "W")
            assert float(pa[1].abs().max()) > 0 and float(pw[1].abs().max()) > 0
            assert float(pw[0].abs().max()) == G.W_SCALE
            planes = {(M, N, Kp): (pa, pw, b, r)}              # (one shape's planes at a time)
        pa, pw, b, r = planes[(M, N, Kp)]
        res = None if gelu else r
        name = f"{M}x{N}x{Kp} hi_only={hi} gelu={gelu}"
        try:
            if M * N <= SMALL_MN:
                _, g, worst = X.three_product_expectation(pa, pw, 1.0 / G.W_SCALE, hi_only=hi, bias=b, res=res)
                assert g == 2.0 ** -12
                how = "evaluated"
            else:
                worst = G.term_bound(pa, pw, 1.0 / G.W_SCALE, hi, bias=b, res=res)
                how = "bounded"
            if not worst < X.LIMIT:
                failures.append(f"{name}: max sum |term| {worst:.3e} granules ({how})")
        except X.InputNotExact as e:
            failures.append(f"{name}: {e}")
        lines.append(f"{name}: {worst:.3g} ({how})")
    print("max sum |term| in granules of 2^-12: " + "; ".join(lines))
    assert not failures, "representatives that are not exact at their K:\n" + "\n".join(failures)


def test_bound_from_the_planes_is_an_upper_bound():
    """term_bound against the full evaluation where both are cheap"""
    for M, N, Kp in ((70, 77, 96), (70, 77, 8256)):
        a, w, b, r = G.operands(M, N, Kp)
        pa, pw = X.split_model(a), X.split_model(w, G.W_SCALE)
        for hi in (False, True):
            _, g, worst = X.three_product_expectation(pa, pw, 1.0 / G.W_SCALE, hi_only=hi, bias=b, res=r)
            top = G.term_bound(pa, pw, 1.0 / G.W_SCALE, hi, bias=b, res=r)
            assert worst * g / 2.0 ** -12 <= top < X.LIMIT, (M, N, Kp, hi, worst, top)


def test_value_check_tells_one_product_from_three_at_long_k():
    """On a long-K representative the hi.hi sum and the three-product sum differ in more than half of the elements: a
    launch that runs the wrong instantiation cannot pass the bit-exact comparison."""
    long_reps = [c for k, c in G.accepted() if c.Kp > 8192 and c.M * c.N <= SMALL_MN]
    assert long_reps
    c = long_reps[0]
    a, w, b, r = G.operands(c.M, c.N, c.Kp)
    pa, pw = X.split_model(a), X.split_model(w, G.W_SCALE)
    e1, _, _ = X.three_product_expectation(pa, pw, 1.0 / G.W_SCALE, hi_only=True, bias=b, res=r)
    e3, _, _ = X.three_product_expectation(pa, pw, 1.0 / G.W_SCALE, hi_only=False, bias=b, res=r)
    share = float((e1 != e3).double().mean())
    print(f"{c.M}x{c.N}x{c.Kp}: hi.hi and three-product expectations differ in {share:.1%} of the elements")
    assert share > 0.5
    # ... and the f16 rounding of the two (what a reduced-precision split output holds) still differs somewhere
    assert bool((e1.float().half() != e3.float().half()).any())
