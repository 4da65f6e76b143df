// The planar point mass (SS = 5, AS = 3, NP = 9) of the tests is the example env the package ships.
#include "../../../mpopis_amd/env_examples/pointmass.hip"
