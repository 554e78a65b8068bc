// Stand-in of this repository for the glm header of the same name (TEST INFRASTRUCTURE): everything lives in glm/glm.hpp.
#pragma once
#include "../glm.hpp"
