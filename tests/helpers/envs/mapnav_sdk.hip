// The waypoint-and-map env (SS = 4, AS = 2, NP = 10, a table) of the tests is the table example the package ships.
#include "../../../mpopis_amd/env_examples/mapnav.hip"
