// Stand-in of this repository for the OpenGL header (TEST INFRASTRUCTURE): see glew.h.
#pragma once
#include "glew.h"
